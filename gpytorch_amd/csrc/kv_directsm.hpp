// Fused covariance MVM of the SPECTRAL-MIXTURE family (KIND_SM), as the reference EXECUTES it (gpytorch/kernels/spectral_mixture_kernel.py:336-352: the
// sum over the Q mixtures comes before the product over the d input dimensions):
//     k(x, x') = Wsum^d  prod_{j<d}  sum_{q<Q}  w^_q  exp(-2 pi^2 sigma_qj^2 tau_j^2)  cos(2 pi mu_qj tau_j),   tau = x - x',  w^ = w / Wsum,  Wsum = sum_q w_q.
// The kernel generates k~ = k / Wsum^d in [-1, 1] (the caller applies Wsum^d where an outputscale is applied), so the hi/lo f16 split and its 2^12 range
// shift see the value range of every other family.  K is SIGNED here: v_cvt_pkrtz rounds toward zero on both signs, so |hi| <= |K|, lo = K - hi has K's
// sign and |lo| < one f16 ulp of hi -- the split is as exact as for K >= 0 (tests/test_sm_cpu.py restates it on the host).
//
// No per-pair cosine: cos(2 pi mu (x_i - x_j)) = c_i c_j + s_i s_j with c = cos(2 pi frac(x mu)), s = sin(2 pi frac(x mu)) prepared per POINT in float64
// (backend.sm_prep: the phase is reduced to [0, 1) before the cosine and before the cast; a float32 phase is off by 1e-2 at |x| = 1000, mu = 5).  The
// prepared row is
//     [ x_j - shift_j (d columns) | sqrt(w^_q) cos, sqrt(w^_q) sin of (q, j) at columns d + 2 (q d + j), + 1 | zeros to a multiple of four ]
// and the block `sm` holds na[q d + j] = -2 pi^2 sigma_qj^2 log2(e): at most 24 floats, read with ordinary (wave-uniform) loads before the loop.
//
// It IS kv_directh_kernel's body (kv_directh_body.inc) with ONE 32-column tile and a LAZY functor: a row is up to 27 columns wide, far beyond the 8 D
// look-ahead registers per half that body keeps for D <= 10, so the functor reads the packed pair of a column from the staged tile where it uses it.
// Per pair of elements and (q, j): one packed multiply-add for the exponent, one v_exp_f32 per element, a packed multiply and a packed multiply-add
// for c_i c_j + s_i s_j, one packed multiply-add into f_j; per j one packed subtraction and one packed multiply (tau^2); then d - 1 packed multiplies.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KSM_COLS = 32;     // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KSM_MAX_DIM = 3;   // input dimensions d
constexpr int ksm_max_q(int d) { return d == 1 ? 8 : 4; }   // mixtures Q: the prepared width d + 2 Q d stays <= 27
constexpr int ksm_width(int q, int d) { return d + 2 * q * d; }
constexpr bool ksm_ok(int q, int d) { return d >= 1 && d <= KSM_MAX_DIM && q >= 1 && q <= ksm_max_q(d); }
// 32-row tiles per wave: two, or one for few output rows -- and at the widest row (Q = 4, d = 3: 27 columns), where two rows of a lane's own columns next
// to 32 accumulators would spill
constexpr int KSM_NI2_MAX_WIDTH = 24;
constexpr int ksm_ni(bool small, int width) { return (small || width > KSM_NI2_MAX_WIDTH) ? 1 : 2; }

struct KvSmArgs : KvhArgs {
  const float* sm;   // [Q d] na[q d + j] = -2 pi^2 sigma_qj^2 log2(e)
};

template <int Q, int DI>
struct DirectSM {
  static constexpr int SPLIT = DI;
  static constexpr bool LAZY = true;
  struct Shape {
    float na[Q * DI];
  };
  static __device__ __forceinline__ Shape shape(const KvSmArgs& ka) {
    Shape s;
#pragma unroll
    for (int k = 0; k < Q * DI; ++k) s.na[k] = pp_uniform(ka.sm[k]);   // scalar registers (common.hpp)
    return s;
  }
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, const Shape& s) {
    f32x2 k = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      const f32x2 df = (f32x2){zi[j], zi[j]} - row(j);
      const f32x2 t2 = df * df;
      f32x2 f = {0.f, 0.f};
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int c = DI + 2 * (q * DI + j);
        // (the 2^12 range shift of the split contraction enters the exponents of the FIRST dimension's factor only)
        const f32x2 arg = __builtin_elementwise_fma(t2, (f32x2)(s.na[q * DI + j]), (f32x2)(j == 0 ? (float)KGH_KSHIFT : 0.f));
        const f32x2 e = {__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
        const f32x2 g = __builtin_elementwise_fma((f32x2){zi[c + 1], zi[c + 1]}, row(c + 1), (f32x2){zi[c], zi[c]} * row(c));
        f = q == 0 ? e * g : __builtin_elementwise_fma(e, g, f);
      }
      k = j == 0 ? f : k * f;
      // a row is up to 27 columns wide: one dimension's 1 + 2 Q column reads are in flight at a time, and its factor is COMPUTED here -- the tie (a
      // volatile asm keeps its place among the barriers) stops the compiler from sinking the arithmetic below later reads, which left every column
      // of a half live at once and spilled them; the sched_barrier stops the scheduler from hoisting the next dimension's reads above it
      mfma_tie(k);
      __builtin_amdgcn_sched_barrier(0);
    }
    return k;
  }
};

// Same launch bounds and waves_per_eu for every instantiation: gpamd_kv_plan (which sees the prepared width only) may query any of that width
template <int Q, int DI, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directsm_kernel(KvSmArgs ka) {
  static_assert(ksm_ok(Q, DI), "the native envelope: d in 1..3, Q <= 8 at d = 1, Q <= 4 at d = 2, 3");
  using GEN = DirectSM<Q, DI>;
  constexpr int D = ksm_width(Q, DI), CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
