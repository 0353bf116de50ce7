// Fused covariance MVM of the GIBBS family (KIND_GIBBS): the non-stationary covariance with an input-dependent lengthscale l(x) of
// gpytorch/kernels/gibbs_kernel.py:64-82 (which forms dist_sq, S, prod, the prefactor and the exponential as n x m tensors),
//     k(x, x') = ( 2 l(x) l(x') / (l(x)^2 + l(x')^2) )^GIBBS_PREFACTOR_EXPONENT  exp( -|x - x'|^2 / (l(x)^2 + l(x')^2) ).
// The exponent of the prefactor is 1/2 for EVERY d, as the reference executes it (Gibbs / Paciorek-Schervish have d/2): positive definite for d = 1, not in
// general for d >= 2 with a varying l.  The constant below is the kernels' one place to switch; families.GIBBS_PREFACTOR_EXPONENT is the Python side's.
//
// The first family whose prepared rows carry PER-POINT parameters (families.gibbs_prep is the one place that writes them):
//     [ a = l^2 | q = 2^(1/4) sqrt(l) | x - shift (d columns) | zeros ],   width 4 (d <= 2) or 8 (d <= 6)
// With S = a_i + a_j, u = rsqrt(S), s = |x_i - x_j|^2:   k = q_i q_j u exp2(-log2(e) s u^2)   (q_i q_j u = sqrt(2 l_i l_j / S); the diagonal is exactly 1).
// a and q come first and the padding behind the coordinates is zero on both sides, so a padding column adds nothing to s: the kernels do not know d and
// exist in two widths.  0 < k <= 1 by AM-GM, so the hi/lo f16 split and its 2^12 range shift (KGH_KSHIFT, the additive constant of the exponent) see
// the value range of every other family.  A row of zeros (the tile rows past the end of a chunk) has q = 0: k = 0 against a valid row, finite.
//
// It IS kv_directh_kernel's body (kv_directh_body.inc) with ONE 32-column tile and a LAZY functor (as kv_directadd.hpp).  Per pair of elements: one packed
// subtraction and one packed multiply(-add) per coordinate column; a packed add (S), one v_rsq_f32 per element, a packed multiply (u^2); a packed
// multiply and ONE packed multiply-add for the exponent; one v_exp_f32 per element; two packed multiplies by q_i q_j and u (+ one for q_i q_j itself).
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KGB_COLS = 32;        // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KGB_MAX_DIM = 6;      // input dimensions d
constexpr float GIBBS_PREFACTOR_EXPONENT = 0.5f;   // as the reference executes it, whatever d (see above); q = (2^(1/2) l)^GIBBS_PREFACTOR_EXPONENT
static_assert(GIBBS_PREFACTOR_EXPONENT == 0.5f, "the kernels form the prefactor as q_i q_j rsqrt(S): another exponent needs another arithmetic");
constexpr bool kgb_width_ok(int width) { return width == 4 || width == 8; }   // the prepared width: 2 + d padded to a multiple of four

template <int W>
struct DirectGibbs {
  static_assert(kgb_width_ok(W), "prepared width 4 (d <= 2) or 8 (d <= 6)");
  static constexpr int SPLIT = W;
  static constexpr bool LAZY = true;
  static __device__ __forceinline__ float shape(const KvhArgs&) { return 0.f; }   // parameter-free: every parameter is in the rows
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, float) {
    const f32x2 S = (f32x2){zi[0], zi[0]} + row(0);
    const f32x2 qq = (f32x2){zi[1], zi[1]} * row(1);
    f32x2 s = {0.f, 0.f};
#pragma unroll
    for (int k = 2; k < W; ++k) {
      const f32x2 df = (f32x2){zi[k], zi[k]} - row(k);
      s = k == 2 ? df * df : __builtin_elementwise_fma(df, df, s);
    }
    const f32x2 u = {__builtin_amdgcn_rsqf(S[0]), __builtin_amdgcn_rsqf(S[1])};
    const f32x2 arg = __builtin_elementwise_fma(s * (u * u), (f32x2)(-LOG2E), (f32x2)((float)KGH_KSHIFT));
    const f32x2 e = {__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
    return (qq * u) * e;
  }
};

// Same launch bounds and waves_per_eu for both widths (those of kv_directadd_kernel)
template <int W, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directgibbs_kernel(KvhArgs ka) {
  using GEN = DirectGibbs<W>;
  constexpr int D = W, CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
