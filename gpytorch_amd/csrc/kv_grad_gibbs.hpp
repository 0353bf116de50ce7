// Fused bilinear derivative of the GIBBS family (kv_directgibbs.hpp has the formula and the row layout [a = l^2 | q | x - shift | zeros]): kv_grad.hpp's
// W tile on v_mfma_f32_32x32x2_f32, consumed in registers.  Every parameter of the family sits behind the per-point lengthscale l_i, so one pass delivers
//     G0  = sum_ij W_ij k_ij                                   (for an outputscale around the family)
//     g_i = sum_j  W_ij dk_ij/dl_i      for EVERY row i,       dk/dl_i = k ( 1/(2 l_i) - l_i u^2 + 2 s l_i u^4 ),   u^2 = 1 / (l_i^2 + l_j^2),  s = |x_i - x_j|^2
// A lane of the W tile owns ONE row i and 16 columns j of each 32 x 32 block, so g_i is a per-lane sum: float over a 64-column step, float64 across
// steps, the two half-waves combined by one lane exchange, then ONE store per row and j chunk into rows[s][i] -- no atomics, bitwise reproducible; the
// chunks are summed in float64 by gibbs_rows_finalize_kernel.  The column side (d/dl_j of the second cloud) is this kernel with the clouds and L, R
// exchanged.  The derivative is exact at i = j of one cloud: s = 0, u^2 = 1 / (2 l^2) and the bracket cancels to rounding.
#pragma once
#include "kv_grad.hpp"
#include "kv_directgibbs.hpp"

namespace gpamd {

struct GradGibbsArgs {
  GradArgs g;     // part: [nrb * S] partial sums of G0; tiles / kparam unused
  double* rows;   // [S][n] partial row sums
};

template <int W>
__global__ __launch_bounds__(256) void kv_grad_gibbs_kernel(GradGibbsArgs ga) {
  static_assert(kgb_width_ok(W), "prepared width 4 (d <= 2) or 8 (d <= 6)");
  const GradArgs& a = ga.g;
  constexpr int DP = W, DQ = DP / 4;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int th = (a.t + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  float* Ls = dyn + (size_t)wave * (2 * th) * 32;
  float* Xj = dyn + (size_t)4 * (2 * th) * 32 + wave * 64 * DP;
  __shared__ double red[4];

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
  const float li = __builtin_sqrtf(xi[0]);   // a_i = l_i^2
  const float half_inv_li = 0.5f / li;
  double g0 = 0.0, gi = 0.0;
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
    float f0 = 0.f, fg = 0.f;
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
        f0 += wk;
        fg = __builtin_fmaf(wk, br, fg);
      }
    }
    g0 += (double)f0;
    gi += (double)fg;
    __builtin_amdgcn_wave_barrier();
  }

  gi += __shfl_xor(gi, 32, 64);   // the two halves of the wave hold the two column halves of the same 32 rows
  if (h == 0 && i < a.n) ga.rows[(int64_t)s * a.n + i] = gi;
  g0 = wave_sum(g0);
  if (lane == 0) red[wave] = g0;
  __syncthreads();
  if (tid == 0) a.part[unit] = red[0] + red[1] + red[2] + red[3];
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
