// Fused bilinear derivative of the SKL family (kv_directskl.hpp has the formula and the row layout [mu - shift | a | b] in blocks of DB columns): the
// functor of kv_grad.hpp's W tile.  What the family's users learn are the per-point parameters themselves -- a free log sigma^2 per training point, or an
// encoder in front of the kernel -- so one pass over all pairs delivers, next to the two scalars
//     G0 = sum_ij W_ij k_ij                     (an outputscale around the family)
//     G1 = sum_ij W_ij k_ij S_ij                (the lengthscale: dk/dl = k S / (2 l^2), S = 2 SKL)
// the gradient with respect to the mean and the variance of EVERY row point,
//     g_mu[i][q] = -(1 / l)   sum_j W_ij k_ij (mu_iq - mu_jq) (b_iq + b_jq)
//     g_a[i][q]  = -(1 / 2 l) sum_j W_ij k_ij [ b_jq - (a_jq + (mu_iq - mu_jq)^2) b_iq^2 ]
//                = -(1 / 2 l) b_iq^2 sum_j W_ij k_ij [ b_jq (a_iq - a_jq)(a_iq + a_jq) - (mu_iq - mu_jq)^2 ]           (a b = 1: no cancellation)
// A lane of the W tile owns ONE row i and 16 columns j of each 32 x 32 block and reads x_j from the wave's LDS tile as a half-wave broadcast, so the
// 2 DB sums of its row are per-lane registers (the tile's ROWS hook): float over a 64-column step, float64 across steps, the two half-waves combined by
// one lane exchange each, the factors that depend on the row alone (-1 / l; -b_i^2 / (2 l)) applied ONCE per row and chunk in float64 (finish), one
// store per sum, row and j chunk into rows[s][r][i].  No atomics: two calls return the same bits; the chunks are summed in float64 in a fixed order
// (gibbs_rows_finalize_kernel over 2 DB n columns).  The column side (the second cloud's gradient) is this kernel with the clouds and L, R exchanged.
// Exact at i = j of one cloud: every difference is zero, k = 1, and the pair adds W_ii to G0 and nothing else.
#pragma once
#include "kv_grad.hpp"
#include "kv_directskl.hpp"

namespace gpamd {

struct GradSklArgs {
  GradArgs g;     // part: [nrb * S][2] partial sums of G0, G1; kparam: the lengthscale; tiles unused
  double* rows;   // [S][2 DB][n] partial row sums
};

template <int W>
struct GradSkl {
  static_assert(ksk_width_ok(W), "prepared width 4 (d = 1), 12 (d <= 4) or 20 (d <= 6)");
  static constexpr int DP = W, DB = ksk_block(W), NG = 2, TILES = 0, ROWS = 2 * DB;
  double* rows;
  float c = 0.f, inv_l = 0.f;   // -log2(e) / (2 l), 1 / l
  __device__ __forceinline__ void begin(const GradArgs& a, const float (&)[DP]) {
    inv_l = 1.0f / a.kparam;
    c = -0.5f * LOG2E * inv_l;
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG], float (&fr)[ROWS]) const {
    float xj[DP];
    grad_load_xj(xjrow, xj);
    float dm[DB], ta[DB], bs[DB];
    float S = 0.f;
#pragma unroll
    for (int q = 0; q < DB; ++q) {
      const float bi = xi[2 * DB + q], bj = xj[2 * DB + q];
      const float da = xi[DB + q] - xj[DB + q];
      dm[q] = xi[q] - xj[q];
      bs[q] = bi + bj;
      const float dm2 = dm[q] * dm[q], dab = da * bj;
      S = __builtin_fmaf(da * dab, bi, S);
      S = __builtin_fmaf(dm2, bs[q], S);
      ta[q] = __builtin_fmaf(dab, xi[DB + q] + xj[DB + q], -dm2);   // b_j (a_i - a_j)(a_i + a_j) - (mu_i - mu_j)^2
    }
    const float wk = w * __builtin_amdgcn_exp2f(S * c);
    f[0] += wk;
    f[1] = __builtin_fmaf(wk, S, f[1]);
#pragma unroll
    for (int q = 0; q < DB; ++q) {
      fr[q] = __builtin_fmaf(wk * dm[q], bs[q], fr[q]);
      fr[DB + q] = __builtin_fmaf(wk, ta[q], fr[DB + q]);
    }
  }
  // the factors of the row alone: g_mu = -(1 / l) sum, g_a = -(b_i^2 / (2 l)) sum
  __device__ __forceinline__ void finish(const float (&xi)[DP], double (&gi)[ROWS]) const {
#pragma unroll
    for (int q = 0; q < DB; ++q) {
      const double bi = (double)xi[2 * DB + q];
      gi[q] *= -(double)inv_l;
      gi[DB + q] *= -0.5 * (double)inv_l * bi * bi;
    }
  }
};

template <int W>
__global__ __launch_bounds__(256) void kv_grad_skl_kernel(GradSklArgs sa) {
  kv_grad_tile(sa.g, GradSkl<W>{sa.rows});
}

}  // namespace gpamd
