// Fused covariance MVM of the NEWTON-GIRARD ADDITIVE family (KIND_NG): Duvenaud's additive GP with interactions,
//     k(x, x') = sum_{n=1..R} sigma_n e_n(z_1, .., z_d),   z_q = k'(|x_q - x'_q|),   k' in {RBF, Matern 1/2, 3/2, 5/2},   R = max_degree <= d,
// e_n the n-th elementary symmetric polynomial (gpytorch/kernels/newton_girard_additive_kernel.py, which forms a d x n x m tensor, R power sums of it
// and R + 1 polynomials of those).  The kernel generates k~ = k / S, S = sum_n sigma_n C(d, n): unit diagonal, values in [0, 1] like every other family;
// the caller applies S where an outputscale is applied.
//
// It IS kv_directadd_kernel (kv_directh_body.inc, ONE 32-column tile, a LAZY functor) with a polynomial in place of the sum: the d one-dimensional
// covariances of a pair are kda_terms (kv_directadd.hpp) with the additive constant 0, then
//     e_0 = 1, e_n = 0;   for q = 0 .. d - 1:  for n = min(q + 1, RC) .. 1:  e_n += z_q e_{n-1}
// -- positive terms only, at most d RC packed multiply-adds -- and k~ = sum_n w_n e_n.  NOT the Newton-Girard power-sum recursion the reference names
// itself after: that one is an alternating sum and cancels in float32.
//
// The weights are a device block of RC floats, w_n = sigma_n / S * 2^KGH_KSHIFT (the range shift of the split contraction rides in them: no
// instruction of its own), zero for n > max_degree; read into scalar registers before the loop.  RC, the degree cap, is a template parameter and R is
// not: RC = min(D, 3) serves every model with max_degree <= 3, RC = D the others (ng_cap) -- 12 (D, RC) pairs instead of 35 (D, R) pairs per base.
#pragma once
#include "kv_directadd.hpp"

namespace gpamd {

constexpr int KNG_COLS = KDA_COLS;   // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KNG_LOW_CAP = 3;
constexpr bool kng_ok(int d, int r) { return kda_dims_ok(d) && r >= 1 && r <= d; }
// the degree cap of the kernel that serves max_degree = r at d dimensions
constexpr int ng_cap(int d, int r) { return r <= KNG_LOW_CAP ? (d < KNG_LOW_CAP ? d : KNG_LOW_CAP) : d; }

struct KvNgArgs : KvhArgs {
  const float* w;   // [RC] w_n = sigma_n / S * 2^KGH_KSHIFT at index n - 1
};

// e[0 .. RC] of the D values z, by the one-pass recursion (e[0] = 1 is never stored: its products are the z themselves)
template <int D, int RC, typename T>
__device__ __forceinline__ void ng_esp(const T (&z)[D], T (&e)[RC + 1]) {
#pragma unroll
  for (int q = 0; q < D; ++q) {
#pragma unroll
    for (int n = (q + 1 < RC ? q + 1 : RC); n >= 1; --n) {
      if (n == 1) e[1] = q == 0 ? z[0] : e[1] + z[q];
      else if (n == q + 1) e[n] = z[q] * e[n - 1];
      else e[n] = __builtin_elementwise_fma(z[q], e[n - 1], e[n]);
    }
  }
}

template <int KB, int D, int RC>
struct DirectNG {
  static_assert(kng_ok(D, RC), "d in 2..8, degree cap in 1..d");
  static constexpr int SPLIT = D;
  static constexpr bool LAZY = true;
  struct Shape {
    float w[RC];
  };
  static __device__ __forceinline__ Shape shape(const KvNgArgs& ka) {
    Shape s;
#pragma unroll
    for (int n = 0; n < RC; ++n) s.w[n] = pp_uniform(ka.w[n]);   // scalar registers (common.hpp)
    return s;
  }
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, const Shape& s) {
    f32x2 z[D], e[RC + 1];
    kda_terms<KB, D>(zi, row, 0.f, z);
    ng_esp<D, RC>(z, e);
    f32x2 k = e[1] * s.w[0];
#pragma unroll
    for (int n = 2; n <= RC; ++n) k = __builtin_elementwise_fma(e[n], (f32x2)(s.w[n - 1]), k);
    return k;
  }
};

// Same launch bounds and waves_per_eu as the additive kernels, for every instantiation: gpamd_kv_plan, which has no block, may query any of a given d
template <int KB, int D, int RC, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directng_kernel(KvNgArgs ka) {
  using GEN = DirectNG<KB, D, RC>;
  constexpr int CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
