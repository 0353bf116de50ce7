// Fused bilinear derivative of the GIBBS family (kv_directgibbs.hpp has the formula and the row layout [a = l^2 | q | x - shift | zeros]): the functor
// of kv_grad.hpp's W tile.  Every parameter of the family sits behind the per-point lengthscale l_i, so one pass delivers
//     G0  = sum_ij W_ij k_ij                                   (for an outputscale around the family)
//     g_i = sum_j  W_ij dk_ij/dl_i      for EVERY row i,       dk/dl_i = k ( 1/(2 l_i) - l_i u^2 + 2 s l_i u^4 ),   u^2 = 1 / (l_i^2 + l_j^2),  s = |x_i - x_j|^2
// A lane of the W tile owns ONE row i and 16 columns j of each 32 x 32 block, so g_i is a per-lane sum (the tile's ROWS hook): float over a 64-column
// step, float64 across steps, the two half-waves combined by one lane exchange, then ONE store per row and j chunk into rows[s][i] -- no atomics,
// bitwise reproducible; the chunks are summed in float64 by gibbs_rows_finalize_kernel.  The column side (d/dl_j of the second cloud) is this kernel
// with the clouds and L, R exchanged.  The derivative is exact at i = j of one cloud: s = 0, u^2 = 1 / (2 l^2) and the bracket cancels to rounding.
#pragma once
#include "kv_grad.hpp"
#include "kv_directgibbs.hpp"

namespace gpamd {

struct GradGibbsArgs {
  GradArgs g;     // part: [nrb * S] partial sums of G0; tiles / kparam unused
  double* rows;   // [S][n] partial row sums
};

template <int W>
struct GradGibbs {
  static_assert(kgb_width_ok(W), "prepared width 4 (d <= 2) or 8 (d <= 6)");
  static constexpr int DP = W, NG = 1, TILES = 0, ROWS = 1;
  double* rows;
  float li = 0.f, half_inv_li = 0.f;
  __device__ __forceinline__ void begin(const GradArgs&, const float (&xi)[DP]) {
    li = __builtin_sqrtf(xi[0]);   // a_i = l_i^2
    half_inv_li = 0.5f / li;
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG], float& fg) const {
    float xj[DP];
    grad_load_xj(xjrow, xj);
    float sq = 0.f;
#pragma unroll
    for (int q = 2; q < DP; ++q) {
      const float df = xi[q] - xj[q];
      sq = __builtin_fmaf(df, df, sq);
    }
    const float u = __builtin_amdgcn_rsqf(xi[0] + xj[0]);
    const float u2 = u * u, su2 = sq * u2;
    const float k = (xi[1] * xj[1]) * u * __builtin_amdgcn_exp2f(-LOG2E * su2);
    const float wk = w * k;
    // 1/(2 l_i) - l_i u^2 + 2 s l_i u^4 = 1/(2 l_i) - l_i u^2 (1 - 2 s u^2)
    const float br = __builtin_fmaf(-li * u2, __builtin_fmaf(-2.f, su2, 1.f), half_inv_li);
    f[0] += wk;
    fg = __builtin_fmaf(wk, br, fg);
  }
};

template <int W>
__global__ __launch_bounds__(256) void kv_grad_gibbs_kernel(GradGibbsArgs ga) {
  kv_grad_tile(ga.g, GradGibbs<W>{ga.rows});
}

// out[i] = sum_u rows[u][i]   (u = column group x j chunk, fixed order -> reproducible)
__global__ __launch_bounds__(256) void gibbs_rows_finalize_kernel(const double* __restrict__ rows, int units, int n, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int u = 0; u < units; ++u) acc += rows[(int64_t)u * n + i];
  out[i] = (float)acc;
}

}  // namespace gpamd
