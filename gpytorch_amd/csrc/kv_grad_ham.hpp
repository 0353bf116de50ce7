// Fused bilinear derivative of the HAMMING family (kv_directham.hpp has the formula and the packed rows): the functor of kv_grad.hpp's W tile.  With
// s = c / alpha and k~ = (1 + s)^(-beta), one pass delivers three sums, float64 accumulation across tiles in a fixed order (no atomics: two calls give
// the same bits):
//     G[0] = sum W k~                                   (for the outputscale slot, which carries k0 = ((1 + alpha) / alpha)^beta)
//     G[1] = sum W s dk~/ds      = sum W k~ (-beta s / (1 + s))        (dk~/dalpha = -G[1] / alpha: s ~ 1 / alpha)
//     G[2] = sum W dk~/dbeta|_s  = sum W k~ (-ln(1 + s))
// One v_log_f32 serves k~ and G[2]; 1 + s >= 1, so the quotient is a v_rcp_f32 without a guard and c = 0 gives exact zeros in G[1] and G[2].
#pragma once
#include "kv_grad.hpp"
#include "kv_directham.hpp"

namespace gpamd {

struct GradHamArgs {
  GradArgs g;              // part: [nrb * S][3]; tiles / kparam unused
  float inv_alpha, beta;
};

template <int W>
struct GradHam {
  static_assert(khm_width_ok(W), "prepared width 4, 8, 16 or 32 dwords (T <= 16, 32, 64, 128)");
  static constexpr int DP = W, NG = 3, TILES = 0, ROWS = 0;
  float inv_alpha, beta;
  __device__ __forceinline__ void begin(const GradArgs&, const float (&)[DP]) {}
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xjrow + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) c = ham_mismatch(xi[4 * q + e], v[e], c);
    }
    const float s = (float)c * inv_alpha, u = 1.0f + s;
    const float l2 = __builtin_amdgcn_logf(u);   // v_log_f32 = log2
    const float wk = w * __builtin_amdgcn_exp2f(-beta * l2);
    f[0] += wk;
    f[1] = __builtin_fmaf(wk, -beta * s * __builtin_amdgcn_rcpf(u), f[1]);
    f[2] = __builtin_fmaf(wk, -0.6931471805599453f * l2, f[2]);
  }
};

template <int W>
__global__ __launch_bounds__(256) void kv_grad_ham_kernel(GradHamArgs ha) {
  kv_grad_tile(ha.g, GradHam<W>{ha.inv_alpha, ha.beta});
}

}  // namespace gpamd
