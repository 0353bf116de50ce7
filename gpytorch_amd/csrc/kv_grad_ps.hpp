// Fused bilinear derivative of the PRODUCT-STRUCTURE family (kv_directps.hpp has the formula and the prepared rows): the functor of kv_grad.hpp's
// W tile.  One pass delivers 1 + D sums, float64 accumulation across tiles in a fixed order (no atomics: two calls give the same bits):
//     G[0]     = sum W k                                   k = exp(-sum_q r_q) prod_q p_nu(r_q),   r_q = |z_iq - z_jq|
//     G[1 + q] = sum W k rho_q,                            rho_q = (dk'/ds)(s_q) s_q / k'(s_q),    s_q = r_q^2
// so that dk/dl_q = scale G[1 + q] (-2 / l_q).  rho_q is a rational function of r_q alone,
//     nu = 1/2: -r / 2        nu = 3/2: -r^2 / (2 (1 + r))        nu = 5/2: -r^2 (1 + r) / (6 (1 + r + r^2 / 3)),
// with denominators >= 1: coincident coordinates (r_q = 0, every pair of the self-diagonal and every pair of lattice points that share a coordinate)
// give an exact zero without a special case, and the pair needs ONE exponential in total.
#pragma once
#include "kv_grad.hpp"
#include "kv_directps.hpp"

namespace gpamd {

template <int KB, int D>
struct GradPs {
  static_assert(kps_base_ok(KB) && kda_dims_ok(D), "base family Matern 1/2, 3/2, 5/2, d in 2..8");
  static constexpr int DP = (D + 3) / 4 * 4, NG = 1 + D, TILES = 0, ROWS = 0;
  __device__ __forceinline__ void begin(const GradArgs&, const float (&)[DP]) {}
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    float xj[DP];
    grad_load_xj(xjrow, xj);
    float r[D], a[D];
#pragma unroll
    for (int q = 0; q < D; ++q) a[q] = r[q] = __builtin_fabsf(xi[q] - xj[q]);
    kps_tree(a, [](float x, float y) { return x + y; });
    float k = __builtin_amdgcn_exp2f(-LOG2E * a[0]);
    float rho[D];
    if constexpr (KB == KIND_MATERN12) {
#pragma unroll
      for (int q = 0; q < D; ++q) rho[q] = -0.5f * r[q];
    } else {
      float p[D];
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const float r2 = r[q] * r[q], p1 = 1.0f + r[q];
        if constexpr (KB == KIND_MATERN32) {
          p[q] = p1;
          rho[q] = -0.5f * r2 * __builtin_amdgcn_rcpf(p1);
        } else {
          p[q] = __builtin_fmaf(r2, 1.0f / 3.0f, p1);
          rho[q] = (-1.0f / 6.0f) * r2 * p1 * __builtin_amdgcn_rcpf(p[q]);
        }
      }
      kps_tree(p, [](float x, float y) { return x * y; });
      k *= p[0];
    }
    const float wk = w * k;
    f[0] += wk;
#pragma unroll
    for (int q = 0; q < D; ++q) f[1 + q] = __builtin_fmaf(wk, rho[q], f[1 + q]);
  }
};

template <int KB, int D>
__global__ __launch_bounds__(256) void kv_grad_ps_kernel(GradArgs a) {
  kv_grad_tile(a, GradPs<KB, D>{});
}

}  // namespace gpamd
