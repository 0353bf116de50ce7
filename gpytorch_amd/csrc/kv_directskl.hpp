// Fused covariance MVM of the SKL family (KIND_SKL): Gaussian-distributed inputs compared by their symmetrized Kullback-Leibler divergence, the reference's
// GaussianSymmetrizedKLKernel over DistributionalInputKernel (gpytorch/kernels/gaussian_symmetrized_kl_kernel.py:8-47, distributional_input_kernel.py:43-48,
// which broadcast about eight n x m x d tensors).  A point is x = [mu (d) | log sigma^2 (d)]; with a = 1e-8 + exp(log sigma^2), b = 1 / a
//     SKL(x, x') = 1/2 sum_q [ a_q / a'_q + a'_q / a_q - 2 + (mu_q - mu'_q)^2 (b_q + b'_q) ],        k = exp(-SKL / l).
//
// The second family whose prepared rows carry PER-POINT parameters (families.skl_prep is the one place that writes them):
//     [ mu - shift (DB columns) | a (DB) | b (DB) | zeros ],   DB = 1, 4, 6 columns per block  ->  width 4 (d = 1), 12 (d <= 4), 20 (d <= 6)
// a and b are formed once per point in float64 and rounded to float32.  Per pair and column, in packed f32, the DIFFERENCE form
//     S += (a_i - a_j)^2 (b_i b_j) + (mu_i - mu_j)^2 (b_i + b_j)          ( a/a' + a'/a - 2 = (a - a')^2 / (a a') )
// which has no cancellation (a_i b_j + a_j b_i - 2 loses every digit for nearly equal variances) and makes the diagonal EXACTLY 1: both differences are
// zero.  A padding column of a block is zero in all three blocks on both sides and adds nothing, so the kernels do not know d and exist per width.  Then
// ONE v_exp_f32 per pair: k = exp2(S c + KGH_KSHIFT) with c = -log2(e) / (2 l), the 1/2 of the divergence, the lengthscale and the split's range shift in
// one multiply-add.  S >= 0, so 0 < k <= 1: the hi/lo f16 split sees the value range of every other family.  A row of zeros (the tile rows past the end of
// a chunk) gives S = mu_i^2 b_i: finite.
//
// It IS kv_directh_kernel's body (kv_directh_body.inc) with ONE 32-column tile and a LAZY functor, as kv_directgibbs.hpp: the functor reads the three
// columns of a pair from the staged tile where it uses them (3 DB ds_read_b64 per pair of elements), and the lane's own row is 3 DB registers per row tile.
// Seven packed instructions per column and pair of elements: two subtractions, two squares, b_i b_j, b_i + b_j and two multiply-adds into S.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KSK_COLS = 32;        // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KSK_MAX_DIM = 6;      // input dimensions d (a point has 2 d columns)
constexpr bool ksk_width_ok(int width) { return width == 4 || width == 12 || width == 20; }   // the prepared width
constexpr int ksk_block(int width) { return width == 4 ? 1 : (width == 12 ? 4 : 6); }        // DB: columns of each of the three blocks
// 32-row tiles per wave: two, or one for few output rows -- and ONE at width 20, where the 36 row values of two tiles next to the operands do not fit two
// waves per SIMD (the compiler reported 256 VGPRs and 88 / 156 bytes of scratch per lane for NI = 2; NI = 1: 252 / 232 VGPRs, none)
constexpr int ksk_ni(bool small, int width) { return (small || width > 12) ? 1 : 2; }

template <int W>
struct DirectSKL {
  static_assert(ksk_width_ok(W), "prepared width 4 (d = 1), 12 (d <= 4) or 20 (d <= 6)");
  static constexpr int DB = ksk_block(W), SPLIT = 3 * DB;
  static constexpr bool LAZY = true;
  // the exponent's factor: -log2(e) / (2 l), l = the lengthscale (kparam)
  static __device__ __forceinline__ float shape(const KvhArgs& ka) { return -0.5f * LOG2E / ka.a.kparam; }
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, float c) {
    f32x2 S = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < DB; ++q) {
      const f32x2 bj = row(2 * DB + q), bi = {zi[2 * DB + q], zi[2 * DB + q]};
      const f32x2 da = (f32x2){zi[DB + q], zi[DB + q]} - row(DB + q);
      const f32x2 dm = (f32x2){zi[q], zi[q]} - row(q);
      S = __builtin_elementwise_fma(da * da, bi * bj, S);
      S = __builtin_elementwise_fma(dm * dm, bi + bj, S);
    }
    const f32x2 arg = __builtin_elementwise_fma(S, (f32x2){c, c}, (f32x2)((float)KGH_KSHIFT));
    return (f32x2){__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
  }
};

// Same launch bounds and waves_per_eu for every width (those of kv_directgibbs_kernel); D = the 3 DB columns that are read: at width 20 the two trailing
// zeros are neither staged nor kept in registers
template <int W, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directskl_kernel(KvhArgs ka) {
  using GEN = DirectSKL<W>;
  constexpr int D = 3 * ksk_block(W), CT = 1;
  static_assert((D + 3) / 4 * 4 == W, "the row stride of the body is the prepared width");
#include "kv_directh_body.inc"
}

}  // namespace gpamd
