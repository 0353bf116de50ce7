// Fused covariance MVM of the PRODUCT-STRUCTURE family (KIND_PS): the tensor-product (separable) Matern covariance
//     k(x, x') = prod_{q<d} k'(|z_q - z'_q|),   k' in {Matern 1/2, 3/2, 5/2},   d in 2..8,
// of gpytorch/kernels/product_structure_kernel.py:70-76 (which forms a d x n x m tensor and multiplies it down).  With r_q = |z_q - z'_q| in prepared
// units (z = sqrt(2 nu) (x - shift) / l_q, the BASE family's rows) and p_nu the Matern polynomial,
//     prod_q p_nu(r_q) e^{-r_q} = exp(-sum_q r_q) prod_q p_nu(r_q):
// ONE v_exp_f32 per pair of elements whatever d (the additive family takes d), no v_sqrt_f32 (one-dimensional distances are |delta|).  A product of
// one-dimensional RBFs is the RBF with per-dimension lengthscales, which has kernels of its own: no RBF base here.
//
// It IS kv_directadd_kernel (kv_directh_body.inc, ONE 32-column tile, a LAZY functor) with a product in place of the sum.  Per pair of elements: D
// packed subtractions; the moduli (packed f32 has no |.| source modifier: one v_and_b32 per element, as in the additive family); the L1 sum of
// |delta_q| (D - 1 packed adds, pairwise); ONE packed multiply-add for the exponent
// KGH_KSHIFT - log2(e) sum -- the 2^12 range shift of the split contraction is its additive constant --; one v_exp_f32 per element; the polynomials
// 1 + r (nu = 3/2: D packed adds) or 1 + r + r^2 / 3 (nu = 5/2: + D packed multiplies and D packed multiply-adds), stage by stage over the dimensions
// as kda_terms does (kv_directadd.hpp); D packed multiplies for the product.  0 < k <= 1 with an exact unit diagonal (every r_q = 0: exp2(12) 1).
//
// The prepared rows have ZERO padding (stride round_up(d, 4)), as the base family's own.  D is a template parameter and the padding is never read; a
// zero column would be neutral anyway (k'(0) = 1), so no NaN marking as in the additive family.
#pragma once
#include "kv_directadd.hpp"

namespace gpamd {

constexpr int KPS_COLS = KDA_COLS;   // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr bool kps_base_ok(int base) { return base >= KIND_MATERN12 && base <= KIND_MATERN52; }

// v[0] = v[0] op v[1] op .. op v[D - 1], pairwise: (v0 op v1) op (v2 op v3) ..; families.ps_cov restates this order
template <int D, typename T, typename F>
__device__ __forceinline__ void kps_tree(T (&v)[D], F op) {
#pragma unroll
  for (int s = 1; s < D; s *= 2) {
#pragma unroll
    for (int j = 0; j + s < D; j += 2 * s) v[j] = op(v[j], v[j + s]);
  }
}

template <int KB, int D>
struct DirectPS {
  static_assert(kps_base_ok(KB) && kda_dims_ok(D), "base family Matern 1/2, 3/2, 5/2, d in 2..8");
  static constexpr int SPLIT = D;
  static constexpr bool LAZY = true;
  static __device__ __forceinline__ float shape(const KvhArgs&) { return 0.f; }   // parameter-free: base family and d are the template arguments
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, float) {
    f32x2 r[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const f32x2 df = (f32x2){zi[j], zi[j]} - row(j);
      r[j] = (f32x2){__builtin_fabsf(df[0]), __builtin_fabsf(df[1])};
    }
    f32x2 a[D];   // pairwise, so that neither the sum nor the product below is one dependent chain of D instructions (kps_tree)
#pragma unroll
    for (int j = 0; j < D; ++j) a[j] = r[j];
    kps_tree(a, [](f32x2 x, f32x2 y) { return x + y; });
    const f32x2 sum = a[0];
    const f32x2 arg = __builtin_elementwise_fma(sum, (f32x2)(-LOG2E), (f32x2)((float)KGH_KSHIFT));
    f32x2 k = {__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
    if constexpr (KB != KIND_MATERN12) {
      f32x2 p[D];
#pragma unroll
      for (int j = 0; j < D; ++j) p[j] = r[j] + 1.0f;
      if constexpr (KB == KIND_MATERN52) {
#pragma unroll
        for (int j = 0; j < D; ++j) p[j] = __builtin_elementwise_fma(r[j] * r[j], (f32x2)(1.0f / 3.0f), p[j]);
      }
      kps_tree(p, [](f32x2 x, f32x2 y) { return x * y; });
      k = k * p[0];
    }
    return k;
  }
};

// Same launch bounds and waves_per_eu as the additive kernels, for every instantiation: the family is PLANNED as the additive family of the same d
template <int KB, int D, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directps_kernel(KvhArgs ka) {
  using GEN = DirectPS<KB, D>;
  constexpr int CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
