// Fused bilinear derivative of the NEWTON-GIRARD ADDITIVE family (kv_directng.hpp has the formula, the normalisation and the weight block): kv_grad.hpp's
// W tile on v_mfma_f32_32x32x2_f32, consumed in registers.  One pass delivers 1 + D + RC sums, float64 accumulation across tiles:
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
__global__ __launch_bounds__(256) void kv_grad_ng_kernel(GradNgArgs na) {
  static_assert(KB >= KIND_RBF && KB <= KIND_MATERN52 && kng_ok(D, RC), "base family RBF / Matern, d in 2..8, degree cap in 1..d");
  const GradArgs& a = na.g;
  constexpr int DP = (D + 3) / 4 * 4, DQ = DP / 4, NG = 1 + D + RC;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int th = (a.t + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  float* Ls = dyn + (size_t)wave * (2 * th) * 32;
  float* Xj = dyn + (size_t)4 * (2 * th) * 32 + wave * 64 * DP;
  __shared__ double red[4][NG];

  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;
  const int jend = min(a.m, jbeg + a.jchunk);
  const int i0 = rb * 128 + wave * 32;
  const int i = i0 + l31;

  for (int c = h; c < 2 * th; c += 2) {
    float v = 0.f;
    if (c < a.t && i < a.n) v = a.Lt[(int64_t)c * a.ldl + i];
    Ls[c * 32 + l31] = v;
  }
  float xi[DP];
  {
    const int ic = min(i, a.n - 1);
#pragma unroll
    for (int q = 0; q < DQ; ++q) {
      f32x4 v = *reinterpret_cast<const f32x4*>(a.X1 + (int64_t)ic * DP + 4 * q);
      xi[4 * q + 0] = v[0]; xi[4 * q + 1] = v[1]; xi[4 * q + 2] = v[2]; xi[4 * q + 3] = v[3];
    }
  }
  float wn[RC + 2];   // wn[n] = w_n, n = 1 .. RC; wn[RC + 1] = 0 closes the adjoint recursion
  constexpr float UNSHIFT = 1.0f / (float)(1 << KGH_KSHIFT);
#pragma unroll
  for (int n = 1; n <= RC; ++n) wn[n] = pp_uniform(na.w[n - 1]) * UNSHIFT;
  wn[0] = 0.f;
  wn[RC + 1] = 0.f;
  double g[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) g[q] = 0.0;
  __builtin_amdgcn_wave_barrier();

  for (int j0 = jbeg; j0 < jend; j0 += 64) {
    {
      const int j = min(j0 + lane, a.m - 1);
#pragma unroll
      for (int q = 0; q < DQ; ++q)
        *reinterpret_cast<f32x4*>(&Xj[lane * DP + 4 * q]) = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * DP + 4 * q);
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const int ja = j0 + l31, jb = j0 + 32 + l31;
    const bool va = ja < jend, vb = jb < jend;
#pragma unroll 4
    for (int c2 = 0; c2 < th; ++c2) {
      const int c = 2 * c2 + h;
      const bool vc = c < a.t;
      const float* rrow = a.Rt + (int64_t)c * a.ldr;
      float ra = (vc && va) ? rrow[ja] : 0.f;
      float rbv = (vc && vb) ? rrow[jb] : 0.f;
      float lb = Ls[c * 32 + l31];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ra, lb, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(rbv, lb, acc1, 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
    float f[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) f[q] = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jr = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float w = half ? acc1[r] : acc0[r];
        float xj[DP];
#pragma unroll
        for (int q = 0; q < DQ; ++q) {
          f32x4 v = *reinterpret_cast<const f32x4*>(&Xj[jr * DP + 4 * q]);
          xj[4 * q + 0] = v[0]; xj[4 * q + 1] = v[1]; xj[4 * q + 2] = v[2]; xj[4 * q + 3] = v[3];
        }
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
    }
#pragma unroll
    for (int q = 0; q < NG; ++q) g[q] += (double)f[q];
    __builtin_amdgcn_wave_barrier();
  }

#pragma unroll
  for (int q = 0; q < NG; ++q) {
    double v = wave_sum(g[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (tid < NG) a.part[(int64_t)unit * NG + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

}  // namespace gpamd
