// RBF kernel with first- and second-derivative observations (the reference's RBFKernelGradGrad, gpytorch/kernels/rbf_kernel_gradgrad.py:60-151),
// matrix-free, on the pieces of kv_rbfgrad.hpp (its product kernel, argument blocks, tiles, prepared points, split-j slabs, `done` flag and finalize
// kernel): this header holds the Hermite mathematics, the observation policy GradGradObs of the product and the bilinear-derivative kernel.
//
// A point has C = 2 d + 1 components: the value (c = 0), d/dx_a (c = a, 1 <= a <= d) and d2/dx_a^2 (c = d + a); row i C + c is component c of point
// i (the reference's ordering after its perfect shuffle).  With u_q = (x_iq - x_jq) / l_q, k = exp(-|u|^2 / 2), derivative orders alpha (row) and
// beta (column) in {0, e_a, 2 e_a} and the probabilists' Hermite polynomials He_n (He_2 = u^2 - 1, He_3 = u^3 - 3u, He_4 = u^4 - 6u^2 + 3, ...):
//     K[(i, alpha), (j, beta)] = k prod_q (-1)^{alpha_q} He_{alpha_q + beta_q}(u_q) / l_q^{alpha_q + beta_q}
// so the whole C x C block of a pair is ONE exp times polynomials and is never stored.  Product with a column r, r~1_a = r_a / l_a,
// r~2_a = r_{d+a} / l_a^2 (He_3 = u He_2 - 2u and He_4 = He_2^2 + 2 - 4u^2 fold the same-dimension entries into one scalar per pair and column):
//     S0         = r_0 + sum_q [ u_q r~1_q + He_2(u_q) r~2_q ]
//     out_i0    += k S0
//     out_ia    += (1 / l_a)   k [ -u_a S0 + r~1_a + 2 u_a r~2_a ]
//     out_i,d+a += (1 / l_a^2) k [ He_2(u_a) S0 - 2 u_a r~1_a + (2 - 4 u_a^2) r~2_a ]
// 9 d + 1 packed FMAs per pair-column; u^2, He_2, 2u and 2 - 4u^2 are formed once per pair for all columns.
//
// Bilinear form with a left vector l (l~1, l~2 scaled like r): with P = l_0 + sum_q [ -u_q l~1_q + He_2(u_q) l~2_q ] (the left twin of S0 = Q) and
//     corr_a = l~1_a r~1_a + 2 u_a (l~1_a r~2_a - l~2_a r~1_a) + (2 - 4 u_a^2) l~2_a r~2_a
//     l^T K r = sum_ij k f,   f = P Q + sum_a corr_a
// d/dl_a replaces He_s(u_a), s the total order in dimension a, by G_s = He_{s+2} + He_s and multiplies by 1 / l_a:
//     G_0 = u^2,  G_1 = u^3 - 2u,  G_2 = u^4 - 5u^2 + 2,  G_3 = u^5 - 9u^3 + 12u,  G_4 = u^6 - 14u^4 + 39u^2 - 12
// With the parts of dimension a split off -- p_a = -u_a l~1_a + He_2 l~2_a, q_a = u_a r~1_a + He_2 r~2_a, P' = P - p_a, Q' = Q - q_a --
//     f^(a) = u_a^2 (P' Q' + sum_{q != a} corr_q) + P' (G_1 r~1_a + G_2 r~2_a) + (-G_1 l~1_a + G_2 l~2_a) Q'
//             - G_2 l~1_a r~1_a + G_3 (l~2_a r~1_a - l~1_a r~2_a) + G_4 l~2_a r~2_a
// and the kernel writes the sums of functions.rbfgrad_hyper_grads:  G[0] = sum k f,  G[1 + a] = -sum k f^(a)  (d/dl_a = -G[1 + a] / l_a).
#pragma once
#include "kv_rbfgrad.hpp"

namespace gpamd {

// widest instantiated column count per d: the accumulator is RP T C packed registers (profiles/rbfgradgrad_resusage.md)
constexpr int krg2_max_t(int d) { return d <= 3 ? 4 : 2; }

// What a pair contributes besides k, formed once for all columns: u, He_2(u), 2u, 2 - 4u^2 per dimension (V: float or packed float2).
template <int D, typename V>
struct GradGradPair {
  static constexpr int C = 2 * D + 1;
  V u[D], h2[D], tu[D], w[D];
  __device__ __forceinline__ explicit GradGradPair(const V (&dl)[D]) {
#pragma unroll
    for (int q = 0; q < D; ++q) {
      u[q] = dl[q];
      const V uu = dl[q] * dl[q];
      h2[q] = uu - (V)(1.f);
      tu[q] = dl[q] + dl[q];
      w[q] = __builtin_elementwise_fma(uu, (V)(-4.f), (V)(2.f));
    }
  }
  // S0 of a column r = [r_0, r~1[D], r~2[D]]
  template <typename R>
  __device__ __forceinline__ V s0(const R (&r)[C]) const {
    V o = (V)(r[0]);
#pragma unroll
    for (int q = 0; q < D; ++q) o = __builtin_elementwise_fma(h2[q], (V)(r[1 + D + q]), __builtin_elementwise_fma(u[q], (V)(r[1 + q]), o));
    return o;
  }
  // acc[c] += k (block row c applied to r)
  template <typename R>
  __device__ __forceinline__ void apply(V k, const R (&r)[C], V (&acc)[C]) const {
    const V s = s0(r);
    acc[0] = __builtin_elementwise_fma(k, s, acc[0]);
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const V r1 = (V)(r[1 + q]), r2 = (V)(r[1 + D + q]);
      const V g = __builtin_elementwise_fma(-u[q], s, __builtin_elementwise_fma(tu[q], r2, r1));
      acc[1 + q] = __builtin_elementwise_fma(k, g, acc[1 + q]);
      const V h = __builtin_elementwise_fma(h2[q], s, __builtin_elementwise_fma(-tu[q], r1, w[q] * r2));
      acc[1 + D + q] = __builtin_elementwise_fma(k, h, acc[1 + D + q]);
    }
  }
};

// 1, 1 / l_a, 1 / l_a^2 of component b
template <int D>
__device__ __forceinline__ float krg2_scale(const float* invl, int b) {
  if (b == 0) return 1.f;
  const float il = invl[b <= D ? b - 1 : b - D - 1];
  return b <= D ? il : il * il;
}

// Observation policy of kv_gradobs_kernel (kv_rbfgrad.hpp): value, gradient and second derivatives of the RBF family.
template <int D_>
struct GradGradObs {
  static constexpr int D = D_, C = 2 * D_ + 1, MAX_T = krg2_max_t(D_);
  static __device__ __forceinline__ float scale(const float* invl, int b) { return krg2_scale<D>(invl, b); }
  struct Pair {
    const f32x2 k;
    const GradGradPair<D, f32x2> pr;
    __device__ __forceinline__ Pair(const f32x2 (&dl)[D], f32x2 sq) : k(GradRadial<KRG_RBF, f32x2>(sq).k), pr(dl) {}
    __device__ __forceinline__ void apply(const float (&r)[C], f32x2 (&acc)[C]) const { pr.apply(k, r, acc); }
  };
};

// ---- bilinear derivative: the 1 + d sums G of the header over all pairs and the t column pairs, in the shape of kv_grad_rbfgrad_kernel: one lane per
// row i, x_j and R_j of one column staged per j tile, float32 within a 256-pair run, float64 across runs and in the workspace, no atomics;
// rbfgrad_finalize_kernel<D> adds the units in a fixed order.
template <int D>
__global__ __launch_bounds__(256) void kv_grad_rbfgradgrad_kernel(GradRgArgs a) {
  constexpr int C = 2 * D + 1, G = D + 1, BN = KRGG_BN, DP = KRG_DP;
  __shared__ __attribute__((aligned(16))) float Xs[BN * DP];
  __shared__ __attribute__((aligned(16))) float Rs[BN * C];
  __shared__ double red[4][G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;
  const int jend = min(a.m, jbeg + a.jchunk);
  const int i = rb * KRGG_BM + tid;
  const bool vi = i < a.n;
  const float invc = a.invc;
  float xi[D], sc[C];
  {
    const int ic = min(i, a.n - 1);
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = a.X1[(int64_t)ic * DP + k] * invc;
#pragma unroll
    for (int b = 0; b < C; ++b) sc[b] = krg2_scale<D>(a.invl, b);
  }
  double g[G];
#pragma unroll
  for (int b = 0; b < G; ++b) g[b] = 0.0;

  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    __syncthreads();
    {
      const int j = j0 + tid;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (j < jend) v = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * DP);
      *reinterpret_cast<f32x4*>(&Xs[4 * tid]) = v * invc;
    }
    const int nvalid = (jend - j0 < BN ? jend - j0 : BN) * C;
    for (int c = 0; c < a.t; ++c) {
      __syncthreads();
      const float* src = a.Rt + (int64_t)c * a.ldr + (int64_t)j0 * C;
      for (int idx = tid; idx < BN * C; idx += 256) Rs[idx] = idx < nvalid ? src[idx] * krg2_scale<D>(a.invl, idx % C) : 0.f;
      __syncthreads();
      float l[C];
#pragma unroll
      for (int b = 0; b < C; ++b) l[b] = vi ? a.Lt[(int64_t)c * a.ldl + (int64_t)i * C + b] * sc[b] : 0.f;
      float f[G];
#pragma unroll
      for (int b = 0; b < G; ++b) f[b] = 0.f;
#pragma unroll 2
      for (int jj = 0; jj < BN; ++jj) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(&Xs[jj * DP]);
        const float xj[4] = {xv[0], xv[1], xv[2], xv[3]};
        float r[C];
#pragma unroll
        for (int b = 0; b < C; ++b) r[b] = Rs[jj * C + b];
        float dl[D];
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          dl[k] = xi[k] - xj[k];
          sq = __builtin_fmaf(dl[k], dl[k], sq);
        }
        const float kv = GradRadial<KRG_RBF, float>(sq).k;
        const GradGradPair<D, float> pr(dl);
        // P, Q, the parts of every dimension and the same-dimension corrections
        float pa[D], qa[D], corr[D];
        float P = l[0], Q = r[0], cs = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float l1 = l[1 + k], l2 = l[1 + D + k], r1 = r[1 + k], r2 = r[1 + D + k];
          pa[k] = __builtin_fmaf(pr.h2[k], l2, -pr.u[k] * l1);
          qa[k] = __builtin_fmaf(pr.h2[k], r2, pr.u[k] * r1);
          corr[k] = __builtin_fmaf(pr.w[k], l2 * r2, __builtin_fmaf(pr.tu[k], __builtin_fmaf(l1, r2, -l2 * r1), l1 * r1));
          P += pa[k];
          Q += qa[k];
          cs += corr[k];
        }
        f[0] = __builtin_fmaf(kv, __builtin_fmaf(P, Q, cs), f[0]);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float l1 = l[1 + k], l2 = l[1 + D + k], r1 = r[1 + k], r2 = r[1 + D + k];
          const float uu = pr.u[k] * pr.u[k], u1 = pr.u[k];
          const float g1 = u1 * (uu - 2.f);                                                                       // u^3 - 2u
          const float g2 = __builtin_fmaf(uu, uu - 5.f, 2.f);                                                     // u^4 - 5u^2 + 2
          const float g3 = u1 * __builtin_fmaf(uu, uu - 9.f, 12.f);                                               // u^5 - 9u^3 + 12u
          const float g4 = __builtin_fmaf(uu, __builtin_fmaf(uu, uu - 14.f, 39.f), -12.f);                        // u^6 - 14u^4 + 39u^2 - 12
          const float Pm = P - pa[k], Qm = Q - qa[k];
          float fa = uu * __builtin_fmaf(Pm, Qm, cs - corr[k]);
          fa = __builtin_fmaf(Pm, __builtin_fmaf(g2, r2, g1 * r1), fa);
          fa = __builtin_fmaf(__builtin_fmaf(g2, l2, -g1 * l1), Qm, fa);
          fa = __builtin_fmaf(-g2, l1 * r1, fa);
          fa = __builtin_fmaf(g3, __builtin_fmaf(l2, r1, -l1 * r2), fa);
          fa = __builtin_fmaf(g4, l2 * r2, fa);
          f[1 + k] = __builtin_fmaf(-kv, fa, f[1 + k]);
        }
      }
#pragma unroll
      for (int b = 0; b < G; ++b) g[b] += (double)f[b];
    }
  }
#pragma unroll
  for (int b = 0; b < G; ++b) {
    const double v = wave_sum(g[b]);
    if (lane == 0) red[wave][b] = v;
  }
  __syncthreads();
  if (tid < G) a.part[(int64_t)unit * G + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

}  // namespace gpamd
