// Structured kernel interpolation (KISS-GP): the two products with the interpolation matrix W of a cloud of n points on a regular grid of
// M = m_0 ... m_{d-1} nodes, d <= 3.  W [n][M] holds 4^d cubic-convolution weights per point (Keys 1981) and is NEVER stored: every kernel recomputes
// a point's stencil base and weights in registers from its d coordinates and the two numbers (g0, h) of each grid axis.
//
//   gather   Out[c][p]  = sum_k  w_pk U[c][node_pk]                 one point per lane, 4^d x TC loads, weights in registers
//   scatter  U[c][node] = sum_{p : node in stencil(p)} w_p,node V[c][p]   one NODE per lane, no atomics
//   grad     dX[p][a]   = sum_c C[c][p] sum_k (dw_pk / dx_a) G[c][node_pk]   one point per lane, the derivative stencil contracted in float64
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
__device__ __forceinline__ void ski_locate_f64(float x, double g0, double h, int m, int& b, double& r, int& pos) {
  double s = ((double)x - g0) / h;
  s = fmin(fmax(s, -2.0), (double)m + 1.0);   // (a NaN or far-out coordinate must not leave the grid; the host refuses such data before any launch)
  const double f = floor(s);
  b = (int)f - 1;
  r = s - f;
  pos = -1;
  if (b < 0) {
    b = 0;
    pos = s > 0.5 ? 1 : 0;
  } else if (b > m - 4) {
    b = m - 4;
    pos = s > (double)m - 1.5 ? 3 : 2;
  }
}

__device__ __forceinline__ void ski_locate(float x, double g0, double h, int m, int& b, float& r, int& pos) {
  double rd;
  ski_locate_f64(x, g0, h, m, b, rd, pos);
  r = (float)rd;
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

// ---- the gradient with respect to the points.  For a bilinear form sum_c l_c^T (W_1 K_UU W_2^T) r_c the derivative with respect to point p of cloud 1
// is  sum_c l_c[p] sum_k (dw_pk / dx_a) G[c][node_pk]  with the grid vectors G = K_UU W_2^T R (and the mirror image for cloud 2).  The derivative of a
// stencil weight is the u'-weight on axis a times the plain weights on the other axes; the per-axis arguments a = r + 1, r, 1 - r, 2 - r have
// da/dr = +1, +1, -1, -1 and dr/dx = 1 / h.  An axis under the boundary rule (one-hot weights) has derivative zero on THAT axis only.  Keys' kernel is
// C^1, so the gradient is continuous across cell edges, and the four derivative weights of an axis sum to zero: a constant G gives zero.
//
// One point per lane in `perm` order, as the gather.  r, the d x 4 weights and the d x 4 derivative weights are float64 registers; the 4^d nodes are
// walked once per group of TC columns (a tail of t % TC columns one by one).  The coefficient C[c][p] belongs to the lane, so the columns are
// contracted FIRST, at every node: H[node] = sum_c C[c][p] G[c][node] (G read as float32, the sum in float64) -- one fma per load and no per-column
// sums to keep -- and the d axis sums then take H through the stencil, the last axis (whose four nodes are neighbours in memory) innermost:
// out[a < L] += (outer factor of axis a) * sum_o w_L[o] H[o],  out[L] += (outer plain factor) * sum_o dw_L[o] H[o].  With two pairs (GA, CA), (GB, CB) --
// x1 is x2 in training: both sides of the bilinear form move the same point -- a node is read from both grid vectors in the same pass.  All t columns
// run inside the kernel and dX is written once: no atomics, no LDS, one fixed summation order, bitwise reproducible.
constexpr int SKI_GC = 4;         // gradient: columns per group

__device__ __forceinline__ double ski_sel4(const double (&v)[4], int o) { return o == 0 ? v[0] : (o == 1 ? v[1] : (o == 2 ? v[2] : v[3])); }

// weight and derivative weight (d/dx) at stencil position o of an axis with spacing h
__device__ __forceinline__ void ski_weight_f64(double r, int pos, double h, int o, double& w, double& dw) {
  const double a = o == 0 ? r + 1.0 : (o == 1 ? r : (o == 2 ? 1.0 - r : 2.0 - r));
  const bool in = o == 1 || o == 2;
  const double u = in ? ((1.5 * a - 2.5) * a) * a + 1.0 : ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
  const double du = in ? (4.5 * a - 5.0) * a : (-1.5 * a + 5.0) * a - 4.0;
  w = pos < 0 ? u : (pos == o ? 1.0 : 0.0);
  dw = pos < 0 ? (o < 2 ? du : -du) / h : 0.0;
}

struct SkiGradArgs {
  const float* X;
  int64_t ldx;
  const int* perm;   // optional, as the gather's
  const float* GA;   // [t][ldg] grid vectors
  const float* CA;   // [t][ldc] per-point coefficients
  const float* GB;   // second pair (TWO), else null
  const float* CB;
  int64_t ldg;
  int64_t ldc;
  float* dX;         // [n][lddx]
  int64_t lddx;
  int n;
  int t;
  SkiGrid g;
};

// columns c0 .. c0 + W of point p added to out[0..D): one walk over the 4^D nodes, as 4^(D-1) rows of four neighbouring nodes
template <int D, int W, bool TWO>
__device__ __forceinline__ void ski_grad_group(const SkiGradArgs& a, int c0, int p, const int (&b)[3], int m1, int m2, const double (&w)[3][4],
                                               const double (&dw)[3][4], double (&out)[3]) {
  constexpr int L = D - 1;   // the last axis: its four nodes are neighbours in memory
  double ca[W], cb[W];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    ca[c] = (double)a.CA[(int64_t)(c0 + c) * a.ldc + p];
    cb[c] = TWO ? (double)a.CB[(int64_t)(c0 + c) * a.ldc + p] : 0.0;
  }
  // (the rows stay a loop: unrolled, the 4^D x W loads are all hoisted and their results no longer fit the registers)
#pragma unroll 1
  for (int row = 0; row < (1 << (2 * L)); ++row) {
    const int oa = row >> 2, ob = row & 3;   // D = 3: (o0, o1); D = 2: (-, o0)
    double fo[3] = {0.0, 0.0, 0.0}, fp = 1.0;   // outer factors: of the derivative along outer axis ax, and of the derivative along the last axis
    int node = 0;
    if (D == 2) {
      fo[0] = ski_sel4(dw[0], ob);
      fp = ski_sel4(w[0], ob);
      node = b[0] + ob;
    } else if (D == 3) {
      const double w0 = ski_sel4(w[0], oa), w1 = ski_sel4(w[1], ob);
      fo[0] = ski_sel4(dw[0], oa) * w1;
      fo[1] = w0 * ski_sel4(dw[1], ob);
      fp = w0 * w1;
      node = (b[0] + oa) * m1 + b[1] + ob;
    }
    node = node * (D > 1 ? (D > 2 ? m2 : m1) : 1) + b[L];
    double hw = 0.0, hd = 0.0;   // sum_o w_L[o] H[o] and sum_o dw_L[o] H[o] over the row's four nodes
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      double hn = 0.0;           // H[node] = sum_c CA[c][p] GA[c][node] (+ CB GB): the columns contracted first
#pragma unroll
      for (int c = 0; c < W; ++c) {
        hn = fma(ca[c], (double)a.GA[(int64_t)(c0 + c) * a.ldg + node + o], hn);
        if (TWO) hn = fma(cb[c], (double)a.GB[(int64_t)(c0 + c) * a.ldg + node + o], hn);
      }
      hw = fma(w[L][o], hn, hw);
      hd = fma(dw[L][o], hn, hd);
    }
#pragma unroll
    for (int ax = 0; ax < L; ++ax) out[ax] = fma(fo[ax], hw, out[ax]);
    out[L] = fma(fp, hd, out[L]);
  }
}

// (four workgroups per CU: the 24 float64 weights and a row's 4 x TC x 2 loads in flight take 130 registers at D = 3 with two pairs unbounded, two over
//  the 128 that four waves per SIMD leave each; bounded, every instantiation fits without scratch)
template <int D, int TC, bool TWO>
__global__ __launch_bounds__(SKI_P, 4) void ski_interp_grad_kernel(SkiGradArgs a) {
  const int i = blockIdx.x * SKI_P + threadIdx.x;
  if (i >= a.n) return;
  const int p = a.perm ? a.perm[i] : i;
  int b[3] = {0, 0, 0};
  double w[3][4], dw[3][4];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (ax < D) {
      int pos;
      double r;
      ski_locate_f64(a.X[(int64_t)p * a.ldx + ax], a.g.g0[ax], a.g.h[ax], a.g.m[ax], b[ax], r, pos);
#pragma unroll
      for (int o = 0; o < 4; ++o) ski_weight_f64(r, pos, a.g.h[ax], o, w[ax][o], dw[ax][o]);
    } else {
#pragma unroll
      for (int o = 0; o < 4; ++o) { w[ax][o] = 1.0; dw[ax][o] = 0.0; }
    }
  }
  const int m1 = D > 1 ? a.g.m[1] : 1, m2 = D > 2 ? a.g.m[2] : 1;
  double out[3] = {0.0, 0.0, 0.0};
  int c0 = 0;
  for (; c0 + TC <= a.t; c0 += TC) ski_grad_group<D, TC, TWO>(a, c0, p, b, m1, m2, w, dw, out);
  for (; c0 < a.t; ++c0) ski_grad_group<D, 1, TWO>(a, c0, p, b, m1, m2, w, dw, out);
#pragma unroll
  for (int ax = 0; ax < D; ++ax) a.dX[(int64_t)p * a.lddx + ax] = (float)out[ax];
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
