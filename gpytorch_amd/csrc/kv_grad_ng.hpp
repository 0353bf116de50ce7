// Fused bilinear derivative of the NEWTON-GIRARD ADDITIVE family (kv_directng.hpp has the formula, the normalisation and the weight block): the functor
// of kv_grad.hpp's W tile.  One pass delivers 1 + D + RC sums, float64 accumulation across tiles:
//     G[0]             = sum W k~                                             k~ = sum_n w_n e_n(z),   w_n = sigma_n / S  (the block's 2^KGH_KSHIFT removed)
//     G[1 + q]         = sum W (dk~/dz_q) (dk'/ds)(s_q) s_q,                  s_q = (z_iq - z_jq)^2,   dk~/dz_q = sum_n w_n e_{n-1}(z without z_q)
//     G[1 + D + n - 1] = sum W e_n                                            n = 1 .. RC  (for the sigma_n)
// The leave-one-out polynomials are the ADJOINT of the forward recursion, never a quotient by z_q (which underflows to 0 for far pairs): with P_q the
// polynomials of z_0 .. z_{q-1} (the states the forward pass goes through) and the adjoint A = w after the last dimension,
//     for q = D - 1 .. 0:   dk~/dz_q = sum_n A_n P_q[n-1];   A_n += z_q A_{n+1}
// -- positive terms only, 2 D RC multiply-adds.  (dk'/ds) s comes from cov_dcov_times_sq (common.hpp): an exact zero at r = 0 for Matern-1/2 too, on
// every pair that shares a coordinate.
#pragma once
#include "kv_grad.hpp"
#include "kv_directng.hpp"

namespace gpamd {

struct GradNgArgs {
  GradArgs g;       // part: [nrb*S][1 + D + RC]; tiles / kparam unused
  const float* w;   // [RC] w_n = sigma_n / S * 2^KGH_KSHIFT at index n - 1 (the block of the product kernel)
};

template <int KB, int D, int RC>
struct GradNg {
  static_assert(KB >= KIND_RBF && KB <= KIND_MATERN52 && kng_ok(D, RC), "base family RBF / Matern, d in 2..8, degree cap in 1..d");
  static constexpr int DP = (D + 3) / 4 * 4, NG = 1 + D + RC, TILES = 0, ROWS = 0;
  const float* block;   // GradNgArgs::w
  float wn[RC + 2];   // wn[n] = w_n, n = 1 .. RC; wn[RC + 1] = 0 closes the adjoint recursion
  __device__ __forceinline__ void begin(const GradArgs&, const float (&)[DP]) {
    constexpr float UNSHIFT = 1.0f / (float)(1 << KGH_KSHIFT);
#pragma unroll
    for (int n = 1; n <= RC; ++n) wn[n] = pp_uniform(block[n - 1]) * UNSHIFT;
    wn[0] = 0.f;
    wn[RC + 1] = 0.f;
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    float xj[DP];
    grad_load_xj(xjrow, xj);
    float z[D], dzs[D];
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const float df = xi[q] - xj[q];
      cov_dcov_times_sq<KB>(df * df, z[q], dzs[q]);
    }
    // forward: P[q][n] = e_n(z_0 .. z_{q-1}), n = 0 .. min(q, RC) (the entries above are zero and never read); P[D] = the e_n themselves
    float P[D + 1][RC + 1];
    P[0][0] = 1.f;
#pragma unroll
    for (int q = 0; q < D; ++q) {
      P[q + 1][0] = 1.f;
#pragma unroll
      for (int n = 1; n <= RC; ++n) {
        if (n > q + 1) continue;
        P[q + 1][n] = (n == q + 1) ? z[q] * P[q][n - 1] : __builtin_fmaf(z[q], P[q][n - 1], P[q][n]);
      }
    }
    float kt = 0.f;
#pragma unroll
    for (int n = 1; n <= RC; ++n) {
      kt = __builtin_fmaf(wn[n], P[D][n], kt);
      f[D + n] = __builtin_fmaf(w, P[D][n], f[D + n]);
    }
    f[0] = __builtin_fmaf(w, kt, f[0]);
    // adjoint, from the last dimension down
    float A[RC + 2];
#pragma unroll
    for (int n = 0; n <= RC + 1; ++n) A[n] = wn[n];
#pragma unroll
    for (int q = D - 1; q >= 0; --q) {
      float dk = 0.f;
#pragma unroll
      for (int n = 1; n <= RC; ++n)
        if (n - 1 <= q) dk = __builtin_fmaf(A[n], P[q][n - 1], dk);
      f[1 + q] = __builtin_fmaf(w * dk, dzs[q], f[1 + q]);
#pragma unroll
      for (int n = 1; n <= RC; ++n) A[n] = __builtin_fmaf(z[q], A[n + 1], A[n]);
    }
  }
};

template <int KB, int D, int RC>
__global__ __launch_bounds__(256) void kv_grad_ng_kernel(GradNgArgs na) {
  kv_grad_tile(na.g, GradNg<KB, D, RC>{na.w, {}});
}

}  // namespace gpamd
