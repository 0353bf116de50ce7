// Fused covariance MVM of the ADDITIVE family (KIND_ADD): k~(x, x') = (1/d) sum_{q<d} k'(|z_q - z'_q|), k' in {RBF, Matern 1/2, 3/2, 5/2}, the first-order
// additive GP of gpytorch/kernels/additive_structure_kernel.py:62-68 (which forms a d x n x m tensor and sums it).  It IS kv_directh_kernel's body
// (kv_directh_body.inc: direct differences on the packed-f32 pipe, contraction of hi/lo-split operands on the f16 matrix pipe) with ONE 32-column tile and
// a LAZY pair functor: the d one-dimensional covariances of a pair of elements are generated from the columns of the staged tile and summed in
// registers, then contracted ONCE -- where the sum of d one-dimensional operators runs the whole product, contraction included, d times.
//
// Per pair of elements and dimension: one packed subtraction; the distance is |delta| (no v_sqrt_f32 in one dimension; RBF takes delta^2 inside its
// exponent's packed multiply-add); one packed multiply-add for the exponent; one v_exp_f32 per element; the Matern polynomial (0 .. 2 packed
// instructions); one packed add into the sum.  The factor 2^12 / d -- the range shift of the split contraction (KGH_KSHIFT) and the mean -- is the
// additive constant 12 - log2(d) of every exponent: no instruction of its own.
//
// The functor reads columns where it uses them (LAZY, as kv_directsm.hpp) at every d: the sum needs each column once, so the 8 D look-ahead registers
// per half of the plain form would only hold values that are consumed immediately.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KDA_COLS = 32;      // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KDA_MIN_DIM = 2, KDA_MAX_DIM = 8;
constexpr bool kda_dims_ok(int d) { return d >= KDA_MIN_DIM && d <= KDA_MAX_DIM; }
constexpr float kda_log2(int d) {
  constexpr float L2[KDA_MAX_DIM + 1] = {0.f, 0.f, 1.f, 1.5849625007211562f, 2.f, 2.321928094887362f, 2.584962500721156f, 2.807354922057604f, 3.f};
  return L2[d];
}

// The d one-dimensional covariances of a pair of elements, e[q] = 2^C k'(|z_iq - z_jq|): shared by the additive functor below and the Newton-Girard
// functor (kv_directng.hpp), so the two cannot drift.  Stage by stage over the d independent dimensions (all differences, all exponents, all
// exponentials, the polynomials): written dimension by dimension every instruction waits on the one before it (cov_pairs_from_sq, common.hpp)
template <int KB, int D, typename R>
__device__ __forceinline__ void kda_terms(const float* zi, R row, float C, f32x2 (&e)[D]) {
  static_assert(KB >= KIND_RBF && KB <= KIND_MATERN52 && kda_dims_ok(D), "base family RBF / Matern, d in 2..8");
  f32x2 df[D];
#pragma unroll
  for (int j = 0; j < D; ++j) df[j] = (f32x2){zi[j], zi[j]} - row(j);
  if constexpr (KB == KIND_RBF) {
#pragma unroll
    for (int j = 0; j < D; ++j) e[j] = __builtin_elementwise_fma(df[j], -df[j], (f32x2)(C));
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) e[j] = __builtin_elementwise_fma((f32x2){__builtin_fabsf(df[j][0]), __builtin_fabsf(df[j][1])}, (f32x2)(-LOG2E), (f32x2)(C));
  }
#pragma unroll
  for (int j = 0; j < D; ++j) e[j] = (f32x2){__builtin_amdgcn_exp2f(e[j][0]), __builtin_amdgcn_exp2f(e[j][1])};
  if constexpr (KB == KIND_MATERN32 || KB == KIND_MATERN52) {
    f32x2 p[D];
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = (f32x2){__builtin_fabsf(df[j][0]), __builtin_fabsf(df[j][1])} + 1.0f;
    if constexpr (KB == KIND_MATERN52) {
#pragma unroll
      for (int j = 0; j < D; ++j) p[j] = __builtin_elementwise_fma(df[j] * df[j], (f32x2)(1.0f / 3.0f), p[j]);
    }
#pragma unroll
    for (int j = 0; j < D; ++j) e[j] = p[j] * e[j];
  }
}

template <int KB, int D>
struct DirectAdd {
  static_assert(KB >= KIND_RBF && KB <= KIND_MATERN52 && kda_dims_ok(D), "base family RBF / Matern, d in 2..8");
  static constexpr int SPLIT = D;
  static constexpr bool LAZY = true;
  static __device__ __forceinline__ float shape(const KvhArgs&) { return 0.f; }   // parameter-free: base family and d are the template arguments
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, float) {
    constexpr float C = (float)KGH_KSHIFT - kda_log2(D);   // every term carries 2^12 / d
    f32x2 e[D];
    kda_terms<KB, D>(zi, row, C, e);
    f32x2 k = e[0];
#pragma unroll
    for (int j = 1; j < D; ++j) k = k + e[j];
    return k;
  }
};

// Same launch bounds and waves_per_eu for every instantiation (those of kv_directp_kernel): gpamd_kv_plan, which has no kparam, may query any of a given d
template <int KB, int D, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directadd_kernel(KvhArgs ka) {
  using GEN = DirectAdd<KB, D>;
  constexpr int CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
