// Fused covariance MVM of the PRODUCT family (KIND_PROD): k(x, x') = k_A(r_A) k_B(r_B) over two column groups of the prepared cloud, A, B in
// {RBF, Matern 1/2, 3/2, 5/2}.  It is kv_directh_kernel (direct differences on the packed-f32 pipe, contraction of hi/lo-split operands on the f16 matrix
// pipe) with ONE 32-column tile and with gen_a accumulating TWO packed squared distances: dimensions [0, DA) -> s_A, [DA, DA + DB) -> s_B, the split a
// compile-time constant of the unrolled loop.  Everything else -- KvhArgs, the V planes and their pre-pass, the column multipliers, the double-buffered
// x_j staging, the pinned software pipeline, mfma_result_fence, the done flag, the tile-list pointer (left null: this family is not culled) -- IS that
// kernel's body (kv_directh_body.inc, included by both).
//
// Cost per pair of elements against the single-family kernel of the same total dimension: the same D packed subtractions and D packed multiply-adds,
// then the second factor -- one more v_sqrt_f32 (Matern), one packed multiply-add for its exponent, one more v_exp_f32 per element, its polynomial
// (0 .. 2 packed instructions) -- and one packed multiply.  The 2^12 range shift of the split contraction (KGH_KSHIFT) enters the FIRST factor's exponent only.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KDP_COLS = 32;      // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KDP_MAX_FACTOR_DIM = 3;

template <int KA, int KB, int DA>
struct DirectProd {
  static_assert(KA >= KIND_RBF && KA <= KB && KB <= KIND_MATERN52 && KB != KIND_RBF, "canonical factor order: K_A <= K_B, not both RBF");
  static constexpr int SPLIT = DA;
  static constexpr bool LAZY = false;
  static __device__ __forceinline__ float shape(const KvhArgs&) { return 0.f; }   // parameter-free factors; the code's content is the template arguments
  static __device__ __forceinline__ f32x2 pair(f32x2 sa, f32x2 sb, float) {
    return cov_pair_from_sq<KA>(sa, 0.f, (float)KGH_KSHIFT) * cov_pair_from_sq<KB>(sb, 0.f, 0.f);
  }
};

// Same launch bounds and waves_per_eu for every instantiation: gpamd_kv_plan (which has no kparam) may query any of a given DA + DB
template <int KA, int KB, int DA, int DB, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directp_kernel(KvhArgs ka) {
  static_assert(DA >= 1 && DA <= KDP_MAX_FACTOR_DIM && DB >= 1 && DB <= KDP_MAX_FACTOR_DIM && (KA != KB || DA <= DB), "the instantiations the code rule admits");
  using GEN = DirectProd<KA, KB, DA>;
  constexpr int D = DA + DB, CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
