// Additive structured kernel interpolation: the two products with W_add = [W_0 | W_1 | .. | W_{d-1}] [n][M], M = sum_q m_q, where W_q interpolates
// column q of the n points onto a ONE-dimensional grid of m_q nodes (g0_q, h_q) -- K = W_add blockdiag(T_q) W_add^T is the covariance of
// AdditiveStructureKernel(GridInterpolationKernel(.., num_dims=1), num_dims=d): 4 d taps per point instead of 4^d.  The d axes are independent and
// travel in the kernel-argument struct; the per-axis rule is kv_ski.hpp's (ski_locate / ski_weight), W is never stored.
//
//   gather   Out[c][p]        = sum_q sum_{o<4} w_{p,q,o} U[c][off_q + b_{p,q} + o]     one point per lane, a runtime loop over q, Out written once
//   scatter  U[c][off_q + j]  = sum_{p : j in stencil_q(p)} w V[c][p]                    one NODE per lane over all M nodes, no atomics
//
// The inverted index is kv_ski.hpp's, per axis and concatenated: axis q's points are sorted (stable) by their clamped stencil base b (0 .. m_q - 4);
// the sorted runs are laid end to end, axis q at positions [q n, (q + 1) n) of `perm` [d n] (values: point numbers), and `cell_start` [cells + 1],
// cells = sum_q (m_q - 3), delimits cell coff_q + b in those positions.
//
// SUMMATION ORDER of the scatter (fixed, so the result is bitwise reproducible).  Node j of axis q adds its cells b = j - o in ascending o = 0..3
// (those with 0 <= b <= m_q - 4).  A cell of at most SKI_LONG points: its points in sorted order, one fma each.  A longer cell: its chunks in chunk
// order, one add per chunk.  A chunk (SKI_LONG consecutive sorted points, one workgroup of ski_add_heavy_kernel): thread (k, sl), k = tid % 4 the
// stencil position, sl = tid / 4 the slice, adds the points begin + sl, begin + sl + 64, .. by fma; the 16 slices of a wave are added by the
// butterfly sl ^ 1, sl ^ 2, sl ^ 4, sl ^ 8 (both partners form the same sum: float addition commutes), the four waves in wave order through LDS.
// On a one-dimensional axis nearly every cell is long once n > SKI_LONG (m - 3): the chunk path is the normal one, d n / SKI_LONG workgroups.
#pragma once
#include "kv_ski.hpp"

namespace gpamd {

constexpr int SKI_ADD_MIN_DIM = 2;
constexpr int SKI_ADD_MAX_DIM = 16;

struct SkiAddGrid {
  double g0[SKI_ADD_MAX_DIM];     // first node of every axis
  double h[SKI_ADD_MAX_DIM];      // spacing
  int m[SKI_ADD_MAX_DIM];         // nodes
  int off[SKI_ADD_MAX_DIM + 1];   // first node of axis q in the concatenation; off[d] = M (entries beyond d: M)
  int coff[SKI_ADD_MAX_DIM + 1];  // first cell of axis q; coff[d] = cells
  int d;
};

struct SkiAddPrepArgs {
  const float* X;
  int64_t ldx;
  int* keys;   // [d][n]
  int n;
  SkiAddGrid g;
};

__global__ __launch_bounds__(256) void ski_add_prepare_kernel(SkiAddPrepArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const float* xr = a.X + (int64_t)p * a.ldx;
  for (int q = 0; q < a.g.d; ++q) {
    int b, pos;
    float r;
    ski_locate(xr[q], a.g.g0[q], a.g.h[q], a.g.m[q], b, r, pos);
    a.keys[(int64_t)q * a.n + p] = b;
  }
}

struct SkiAddGatherArgs {
  const float* X;
  int64_t ldx;
  const int* perm;   // optional [n]: lane i takes point perm[i]
  const float* U;
  int64_t ldg;
  float* Out;
  int64_t ld;
  int n;
  SkiAddGrid g;
};

template <int TC>
__global__ __launch_bounds__(SKI_P) void ski_add_gather_kernel(SkiAddGatherArgs a) {
  const int i = blockIdx.x * SKI_P + threadIdx.x;
  if (i >= a.n) return;
  const int p = a.perm ? a.perm[i] : i;
  const float* xr = a.X + (int64_t)p * a.ldx;
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
  for (int q = 0; q < a.g.d; ++q) {
    int b, pos;
    float r;
    ski_locate(xr[q], a.g.g0[q], a.g.h[q], a.g.m[q], b, r, pos);
    const float* u = a.U + a.g.off[q] + b;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float w = ski_weight(r, pos, o);
#pragma unroll
      for (int c = 0; c < TC; ++c) acc[c] = fmaf(w, u[(int64_t)c * a.ldg + o], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < TC; ++c) a.Out[(int64_t)c * a.ld + p] = acc[c];
}

struct SkiAddScatterArgs {
  const float* X;
  int64_t ldx;
  const int* perm;         // [d n] the points of every axis in cell order
  const int* cell_start;   // [cells + 1] positions in perm
  const int* chunk_off;    // [cells + 1] first chunk of each cell (long cells only have chunks), or null: no long cell
  const int* chunk_begin;  // [chunks] range of each chunk in perm
  const int* chunk_end;
  const float* V;
  int64_t ldv;
  float* U;
  int64_t ldg;
  float* H;                // [chunks][4][hstride]
  int64_t hstride;
  int n;
  int M;
  SkiAddGrid g;
};

// the weight of point p on axis q at stencil position o
__device__ __forceinline__ float ski_add_point_weight(const SkiAddScatterArgs& a, int p, int q, double g0, double h, int m, int o) {
  int b, pos;
  float r;
  ski_locate(a.X[(int64_t)p * a.ldx + q], g0, h, m, b, r, pos);
  return ski_weight(r, pos, o);
}

template <int TC>
__global__ __launch_bounds__(256) void ski_add_heavy_kernel(SkiAddScatterArgs a) {
  constexpr int SL = 64;   // point slices: 16 per wave
  __shared__ float red[TC * 16];
  const int ch = blockIdx.x;
  const int begin = a.chunk_begin[ch], end = a.chunk_end[ch];
  const int q = begin / a.n;   // (a chunk lies inside one axis' run [q n, (q + 1) n))
  const double g0 = a.g.g0[q], h = a.g.h[q];
  const int m = a.g.m[q];
  const int k = threadIdx.x & 3, sl = threadIdx.x >> 2;
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
  for (int s = begin + sl; s < end; s += SL) {
    const int p = a.perm[s];
    const float wt = ski_add_point_weight(a, p, q, g0, h, m, k);
#pragma unroll
    for (int c = 0; c < TC; ++c) acc[c] = fmaf(wt, a.V[(int64_t)c * a.ldv + p], acc[c]);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < TC; ++c) {
#pragma unroll
    for (int s = 4; s < 64; s <<= 1) acc[c] += __shfl_xor(acc[c], s, 64);
    if (lane < 4) red[c * 16 + wave * 4 + lane] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
#pragma unroll
    for (int c = 0; c < TC; ++c) {
      float s = red[c * 16 + k];
      for (int w = 1; w < 4; ++w) s += red[c * 16 + w * 4 + k];
      a.H[((int64_t)ch * 4 + k) * a.hstride + c] = s;
    }
  }
}

template <int TC>
__global__ __launch_bounds__(SKI_G) void ski_add_scatter_kernel(SkiAddScatterArgs a) {
  const int node = blockIdx.x * SKI_G + threadIdx.x;
  if (node >= a.M) return;
  int q = 0;
  while (q + 1 < a.g.d && node >= a.g.off[q + 1]) ++q;
  const int j = node - a.g.off[q], m = a.g.m[q], cbase = a.g.coff[q];
  const double g0 = a.g.g0[q], h = a.g.h[q];
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
  for (int o = 0; o < 4; ++o) {
    const int b = j - o;
    if (b < 0 || b > m - 4) continue;
    const int cell = cbase + b;
    const int cs = a.cell_start[cell], ce = a.cell_start[cell + 1];
    if (a.chunk_off != nullptr && ce - cs > SKI_LONG) {
      const int c1 = a.chunk_off[cell + 1];
      for (int ch = a.chunk_off[cell]; ch < c1; ++ch) {
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] += a.H[((int64_t)ch * 4 + o) * a.hstride + c];
      }
    } else {
      for (int s = cs; s < ce; ++s) {
        const int p = a.perm[s];
        const float wt = ski_add_point_weight(a, p, q, g0, h, m, o);
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = fmaf(wt, a.V[(int64_t)c * a.ldv + p], acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TC; ++c) a.U[(int64_t)c * a.ldg + node] = acc[c];
}

}  // namespace gpamd
