// Fused covariance MVM for clouds OUTSIDE the accuracy policy of the quadratic expansion: squared distances by DIRECT differences on the
// packed-f32 vector pipe, contraction of hi/lo-split operands on the f16 matrix pipe (the contraction half of kv_gramh.hpp).
//
// Why.  Until round 5 every product whose rows could not be block-centred (backend.gram_mode == 0: short lengthscales on curve-like or very
// sparse clouds, Matern nu = 1/2; and the WIDE rows of a block-centred product) ran on kernels that carry the contraction on the VALU
// (kv_valu.hpp, <= 16 columns: D + T/2 packed instructions per pair) or on v_mfma_f32_32x32x2_f32 (kv_mfma.hpp, 1024 matrix-pipe cycles per
// 32 x 32 block and 32-column tile).  With the default ten probe vectors + y that is 11 multiply-adds per pair against ~6 instructions of
// generation: the contraction is two thirds of the VALU work (road3d-shaped workload: 23-28 ms per product, 87 % of a training iteration,
// profiles/r05_s4_workload_road3d_kernel_stats.csv).  The split contraction moves it to three v_mfma_f32_32x32x16_f16 per 16 contracted rows
// (192 matrix-pipe cycles per block) at the price of 2 VALU instructions per pair for the hi/lo split of K.
//
// Layout.  Exactly kv_gramh.hpp's: lane (h, i = l31) of a wave owns the 16 pairs (j(r, h), i), r = 0..15, j(r, h) = (r & 3) + 8 (r >> 2) + 4 h, of a
// 32 x 32 block, i.e. the eight B-operand slots of contraction MFMA mf = r >> 3; the V planes, the pre-pass (kv_vsplit.hpp), the column
// multipliers and the partial-slab convention are shared with that kernel (KvhArgs).  What differs is where S comes from: the x_j rows of a tile
// are staged TRANSPOSED in LDS (Xf[k][j], float), so that one ds_read_b128 per dimension returns the four CONSECUTIVE rows j(4 q .. 4 q + 3, h)
// of a quad -- adjacent register pairs = the two operands of v_pk_add_f32 / v_pk_fma_f32 -- and all lanes of a half-wave read the same address
// (broadcast, conflict-free).  Per pair of elements: D packed subtractions + D packed multiply-adds, then cov_pair_from_sq and the split as in
// kv_gramh.hpp.  One or two 32-column tiles + an optional extra column on the VALU (round 6: K is generated ONCE for up to 65 columns; until then
// 33-65 columns went in groups of 32 and regenerated K for each).
//
// Software pipeline: as kv_gramh.hpp -- the B operands of step s + 1 are generated between the MFMAs of step s (sched_barrier-pinned slices); the
// x_j rows are staged one tile ahead (double-buffered), the V planes per tile.  The loop is VALU-bound (D = 3 Matern-5/2: ~110 VALU instructions
// against 6 MFMAs = 192 cycles per block), so the MFMAs ride for free; what the kernel buys is the VALU work it no longer does.
#pragma once
#include "kv_gramh.hpp"

namespace gpamd {

constexpr int KDH_MAX_DIM = 10;   // instantiated for D in {1,2,3,4,5,6,8,10}: beyond, the per-half x_j registers (8 D) no longer fit next to the operands
constexpr int KDH_COLS = 64;      // columns per launch group (+ 1 extra VALU column): one or two 32-column tiles, K generated ONCE for all of them
// 32-row tiles per wave: two, or one for few output rows -- and with TWO column tiles beyond four dimensions, where 64 accumulators next to the
// 8 D per-half x_j registers of two row tiles would not fit two waves per SIMD
constexpr int kdh_ni(bool small, int ct = 1, int dk = 1) { return (small || (ct == 2 && dk > 4)) ? 1 : 2; }
inline int kdh_bm(int ni) { return 4 * ni * 32; }

// What a pair of squared distances becomes: one family over all D dimensions.  SPLIT: gen_a accumulates dimensions [0, SPLIT) into the first squared
// distance and [SPLIT, D) into a second one (a compile-time split of an unrolled loop: no branch) -- here there is no second group; the product of two
// families over two column groups is kv_directp.hpp's functor
template <int KIND, int D>
struct DirectOne {
  static constexpr int SPLIT = D;
  static constexpr bool LAZY = false;   // the x_j rows of a half travel in registers, loaded one step ahead (kv_directh_body.inc)
  static __device__ __forceinline__ auto shape(const KvhArgs& ka) { return cov_shape<KIND>(ka.a.kparam); }   // the family's shape parameter as the pair functor takes it (common.hpp)
  template <typename S>
  static __device__ __forceinline__ f32x2 pair(f32x2 s2, f32x2, const S& kshape) { return cov_pair_from_sq<KIND>(s2, kshape, (float)KGH_KSHIFT); }
};

template <int KIND, int D, int NI, int CT = 1, int EX = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directh_kernel(KvhArgs ka) {
  using GEN = DirectOne<KIND, D>;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
