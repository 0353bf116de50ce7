// Structured kernel interpolation (KISS-GP): the two products with the interpolation matrix W of a cloud of n points on a regular grid of
// M = m_0 ... m_{d-1} nodes, d <= 3.  W [n][M] holds 4^d cubic-convolution weights per point (Keys 1981) and is NEVER stored: every kernel recomputes
// a point's stencil base and weights in registers from its d coordinates and the two numbers (g0, h) of each grid axis.
//
//   gather   Out[c][p]  = sum_k  w_pk U[c][node_pk]                 one point per lane, 4^d x TC loads, weights in registers
//   scatter  U[c][node] = sum_{p : node in stencil(p)} w_p,node V[c][p]   one NODE per lane, no atomics
//
// The scatter is the inverted-index form: the points are sorted (stable) by the key of their clamped stencil base, key = sum_i b_i prod_{j>i} (m_j - 3),
// and `cell_start` [cells + 1] delimits each cell's run in the sorted order.  Node (j_0, .., j_{d-1}) lies in the stencils of exactly the cells
// b_i = j_i - o_i, o_i = 0..3, that exist (0 <= b_i <= m_i - 4: the boundary rule clamps the base, so keying on the CLAMPED base puts the first and
// last cells of an axis where their stencils are).  The lane walks those cells in ascending (o_0, o_1, o_2) and each cell's points in sorted order,
// recomputes the one weight it needs and adds: a fixed order, so the result is bitwise reproducible.
//
// Long lists: a cell with more than SKI_LONG points (clustered data) is not walked by the node lanes.  Its run is cut into chunks of SKI_LONG
// points; ski_heavy_kernel gives each chunk one workgroup that forms the chunk's 4^d x TC stencil sums (lanes = stencil position x point slice,
// slices added in slice order through LDS) into the workspace H [chunk][4^d][t], and the node lanes add a long cell's chunk sums in chunk order.
//
// Index arithmetic is float64 on the float32 coordinates (three double operations per axis and point): s = (x - g0) / h, f = floor(s), r = s - f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpamd {

constexpr int SKI_MAX_DIM = 3;
constexpr int SKI_P = 256;        // gather: points per workgroup
constexpr int SKI_G = 256;        // scatter: nodes per workgroup
constexpr int SKI_C = 4;          // columns per launch group (t > SKI_C runs as groups)
constexpr int SKI_LONG = 256;     // a cell's list longer than this is summed in chunks of this many points
constexpr int64_t SKI_MAX_NODES = (int64_t)1 << 24;

struct SkiGrid {
  double g0[SKI_MAX_DIM];   // first node of the axis
  double h[SKI_MAX_DIM];    // spacing
  int m[SKI_MAX_DIM];       // nodes
};

// Where x sits on one axis: the clamped stencil base b (0 .. m - 4), the fractional offset r and `pos`: -1 inside, else the stencil position of
// the one-hot weight of the boundary rule (the node among the first / last four nearest to x).
__device__ __forceinline__ void ski_locate(float x, double g0, double h, int m, int& b, float& r, int& pos) {
  double s = ((double)x - g0) / h;
  s = fmin(fmax(s, -2.0), (double)m + 1.0);   // (a NaN or far-out coordinate must not leave the grid; the host refuses such data before any launch)
  const double f = floor(s);
  b = (int)f - 1;
  r = (float)(s - f);
  pos = -1;
  if (b < 0) {
    b = 0;
    pos = s > 0.5 ? 1 : 0;
  } else if (b > m - 4) {
    b = m - 4;
    pos = s > (double)m - 1.5 ? 3 : 2;
  }
}

// weight at stencil position o (0..3): u(r + 1), u(r), u(r - 1), u(r - 2) of Keys' cubic convolution, or the one-hot boundary weight
__device__ __forceinline__ float ski_weight(float r, int pos, int o) {
  const float a = o == 0 ? r + 1.f : (o == 1 ? r : (o == 2 ? 1.f - r : 2.f - r));
  const float inner = ((1.5f * a - 2.5f) * a) * a + 1.f;
  const float outer = ((-0.5f * a + 2.5f) * a - 4.f) * a + 2.f;
  const float w = (o == 1 || o == 2) ? inner : outer;
  return pos < 0 ? w : (pos == o ? 1.f : 0.f);
}

struct SkiPrepArgs {
  const float* X;
  int64_t ldx;
  int* keys;
  int n;
  SkiGrid g;
};

template <int D>
__global__ __launch_bounds__(256) void ski_prepare_kernel(SkiPrepArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  int key = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    int b, pos;
    float r;
    ski_locate(a.X[(int64_t)p * a.ldx + i], a.g.g0[i], a.g.h[i], a.g.m[i], b, r, pos);
    key = key * (a.g.m[i] - 3) + b;
  }
  a.keys[p] = key;
}

struct SkiGatherArgs {
  const float* X;
  int64_t ldx;
  const int* perm;   // optional: lane i takes point perm[i] (neighbouring lanes then read neighbouring nodes)
  const float* U;
  int64_t ldg;
  float* Out;
  int64_t ld;
  int n;
  SkiGrid g;
};

template <int D, int TC>
__global__ __launch_bounds__(SKI_P) void ski_gather_kernel(SkiGatherArgs a) {
  const int i = blockIdx.x * SKI_P + threadIdx.x;
  if (i >= a.n) return;
  const int p = a.perm ? a.perm[i] : i;
  int b[3] = {0, 0, 0};
  float w[3][4];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (ax < D) {
      int pos;
      float r;
      ski_locate(a.X[(int64_t)p * a.ldx + ax], a.g.g0[ax], a.g.h[ax], a.g.m[ax], b[ax], r, pos);
#pragma unroll
      for (int o = 0; o < 4; ++o) w[ax][o] = ski_weight(r, pos, o);
    } else {
#pragma unroll
      for (int o = 0; o < 4; ++o) w[ax][o] = 1.f;
    }
  }
  const int m1 = D > 1 ? a.g.m[1] : 1, m2 = D > 2 ? a.g.m[2] : 1;
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
#pragma unroll
  for (int o0 = 0; o0 < 4; ++o0) {
#pragma unroll
    for (int o1 = 0; o1 < (D > 1 ? 4 : 1); ++o1) {
#pragma unroll
      for (int o2 = 0; o2 < (D > 2 ? 4 : 1); ++o2) {
        float wt = w[0][o0];
        if (D > 1) wt *= w[1][o1];
        if (D > 2) wt *= w[2][o2];
        int node = b[0] + o0;
        if (D > 1) node = node * m1 + b[1] + o1;
        if (D > 2) node = node * m2 + b[2] + o2;
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = fmaf(wt, a.U[(int64_t)c * a.ldg + node], acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TC; ++c) a.Out[(int64_t)c * a.ld + p] = acc[c];
}

struct SkiScatterArgs {
  const float* X;
  int64_t ldx;
  const int* perm;         // [n] the points in cell order
  const int* cell_start;   // [cells + 1]
  const int* chunk_off;    // [cells + 1] first chunk of each cell (long cells only have chunks), or null: no long cell
  const int* chunk_begin;  // [chunks] range of each chunk in the sorted order
  const int* chunk_end;
  const float* V;
  int64_t ldv;
  float* U;
  int64_t ldg;
  float* H;                // [chunks][4^D][hstride]
  int64_t hstride;
  int M;
  SkiGrid g;
};

// the product of the D per-axis weights of point p at stencil position (o0, o1, o2)
template <int D>
__device__ __forceinline__ float ski_point_weight(const SkiScatterArgs& a, int p, int o0, int o1, int o2) {
  float wt = 1.f;
#pragma unroll
  for (int ax = 0; ax < D; ++ax) {
    int b, pos;
    float r;
    ski_locate(a.X[(int64_t)p * a.ldx + ax], a.g.g0[ax], a.g.h[ax], a.g.m[ax], b, r, pos);
    const float w = ski_weight(r, pos, ax == 0 ? o0 : (ax == 1 ? o1 : o2));
    wt = ax == 0 ? w : wt * w;
  }
  return wt;
}

template <int D, int TC>
__global__ __launch_bounds__(256) void ski_heavy_kernel(SkiScatterArgs a) {
  constexpr int NS = 1 << (2 * D);   // stencil positions
  constexpr int SL = 256 / NS;       // point slices
  __shared__ float red[TC * 256];
  const int ch = blockIdx.x;
  const int begin = a.chunk_begin[ch], end = a.chunk_end[ch];
  const int k = threadIdx.x % NS, sl = threadIdx.x / NS;
  const int o0 = (k >> (2 * (D - 1))) & 3, o1 = D > 1 ? (k >> (2 * (D - 2))) & 3 : 0, o2 = D > 2 ? k & 3 : 0;
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
  for (int q = begin + sl; q < end; q += SL) {
    const int p = a.perm[q];
    const float wt = ski_point_weight<D>(a, p, o0, o1, o2);
#pragma unroll
    for (int c = 0; c < TC; ++c) acc[c] = fmaf(wt, a.V[(int64_t)c * a.ldv + p], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < TC; ++c) red[c * 256 + threadIdx.x] = acc[c];
  __syncthreads();
  if (sl == 0) {
#pragma unroll
    for (int c = 0; c < TC; ++c) {
      float s = 0.f;
      for (int j = 0; j < SL; ++j) s += red[c * 256 + j * NS + k];
      a.H[((int64_t)ch * NS + k) * a.hstride + c] = s;
    }
  }
}

template <int D, int TC>
__global__ __launch_bounds__(SKI_G) void ski_scatter_kernel(SkiScatterArgs a) {
  constexpr int NS = 1 << (2 * D);
  const int node = blockIdx.x * SKI_G + threadIdx.x;
  if (node >= a.M) return;
  const int m0 = a.g.m[0], m1 = D > 1 ? a.g.m[1] : 1, m2 = D > 2 ? a.g.m[2] : 1;
  int j0, j1 = 0, j2 = 0;
  {
    int rest = node;
    if (D > 2) { j2 = rest % m2; rest /= m2; }
    if (D > 1) { j1 = rest % m1; rest /= m1; }
    j0 = rest;
  }
  float acc[TC];
#pragma unroll
  for (int c = 0; c < TC; ++c) acc[c] = 0.f;
  for (int o0 = 0; o0 < 4; ++o0) {
    for (int o1 = 0; o1 < (D > 1 ? 4 : 1); ++o1) {
      for (int o2 = 0; o2 < (D > 2 ? 4 : 1); ++o2) {
        const int b0 = j0 - o0, b1 = j1 - o1, b2 = j2 - o2;
        bool ok = b0 >= 0 && b0 <= m0 - 4;
        if (D > 1) ok = ok && b1 >= 0 && b1 <= m1 - 4;
        if (D > 2) ok = ok && b2 >= 0 && b2 <= m2 - 4;
        if (!ok) continue;
        int cell = b0;
        if (D > 1) cell = cell * (m1 - 3) + b1;
        if (D > 2) cell = cell * (m2 - 3) + b2;
        const int cs = a.cell_start[cell], ce = a.cell_start[cell + 1];
        if (a.chunk_off != nullptr && ce - cs > SKI_LONG) {
          const int k = D == 1 ? o0 : (D == 2 ? o0 * 4 + o1 : (o0 * 4 + o1) * 4 + o2);
          const int c1 = a.chunk_off[cell + 1];
          for (int ch = a.chunk_off[cell]; ch < c1; ++ch) {
#pragma unroll
            for (int c = 0; c < TC; ++c) acc[c] += a.H[((int64_t)ch * NS + k) * a.hstride + c];
          }
        } else {
          for (int q = cs; q < ce; ++q) {
            const int p = a.perm[q];
            const float wt = ski_point_weight<D>(a, p, o0, o1, o2);
#pragma unroll
            for (int c = 0; c < TC; ++c) acc[c] = fmaf(wt, a.V[(int64_t)c * a.ldv + p], acc[c]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TC; ++c) a.U[(int64_t)c * a.ldg + node] = acc[c];
}

}  // namespace gpamd
