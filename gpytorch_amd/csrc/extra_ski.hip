// extern "C" entry points of structured kernel interpolation (kv_ski.hpp): cell keys, W U (gather), W^T V (scatter without atomics) and the gradient
// with respect to the points (the derivative stencil contracted with grid vectors); and of its
// additive form over d one-dimensional axes (kv_ski_add.hpp).
#include "host.hpp"
#include "kv_ski.hpp"
#include "kv_ski_add.hpp"

using namespace gpamd;

namespace {

// validates the grid description (host arrays) and fills the kernels' copy; `what` names the entry point in the message
int ski_grid(const char* what, int d, const double* g0, const double* h, const int* m, SkiGrid* g, int64_t* nodes, int64_t* cells) {
  if (d < 1 || d > SKI_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, what, "d must be in 1..3");
  if (!g0 || !h || !m) return fail(GPAMD_EINVAL, what, "null pointer (grid description)");
  int64_t M = 1, cl = 1;
  for (int i = 0; i < SKI_MAX_DIM; ++i) {
    g->g0[i] = 0.0; g->h[i] = 1.0; g->m[i] = 4;
  }
  for (int i = 0; i < d; ++i) {
    if (m[i] < 4) return fail(GPAMD_EINVAL, what, "every grid axis needs at least 4 nodes");
    if (!(h[i] > 0.0) || !std::isfinite(h[i]) || !std::isfinite(g0[i])) return fail(GPAMD_EINVAL, what, "the grid spacing must be positive and finite");
    M *= m[i];
    cl *= m[i] - 3;
    if (M > SKI_MAX_NODES) return fail(GPAMD_EUNSUPPORTED, what, "the grid has more than 2^24 nodes");
    g->g0[i] = g0[i]; g->h[i] = h[i]; g->m[i] = m[i];
  }
  *nodes = M;
  *cells = cl;
  return 0;
}

// columns of the next launch: the kernels are instantiated for exactly 1, 2 and SKI_C columns (t = 7 runs as 4 + 2 + 1)
int group_width(int left) { return left >= SKI_C ? SKI_C : (left >= 2 ? 2 : 1); }

template <typename F>
void with_d_tc(int d, int tc, F&& f) {
  auto on_tc = [&](auto DD) {
    switch (tc) {
      case 1: f(DD, std::integral_constant<int, 1>{}); break;
      case 2: f(DD, std::integral_constant<int, 2>{}); break;
      default: f(DD, std::integral_constant<int, SKI_C>{}); break;
    }
  };
  switch (d) {
    case 1: on_tc(std::integral_constant<int, 1>{}); break;
    case 2: on_tc(std::integral_constant<int, 2>{}); break;
    default: on_tc(std::integral_constant<int, 3>{}); break;
  }
}

// the additive twin of ski_grid: d independent one-dimensional axes, concatenated
int ski_add_grid(const char* what, int d, const double* g0, const double* h, const int* m, SkiAddGrid* g) {
  if (d < SKI_ADD_MIN_DIM || d > SKI_ADD_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, what, "d must be in 2..16");
  if (!g0 || !h || !m) return fail(GPAMD_EINVAL, what, "null pointer (grid description)");
  int64_t M = 0, cells = 0;
  for (int i = 0; i < SKI_ADD_MAX_DIM; ++i) {
    g->g0[i] = 0.0; g->h[i] = 1.0; g->m[i] = 4;
  }
  for (int i = 0; i < d; ++i) {
    if (m[i] < 4) return fail(GPAMD_EINVAL, what, "every grid axis needs at least 4 nodes");
    if (!(h[i] > 0.0) || !std::isfinite(h[i]) || !std::isfinite(g0[i])) return fail(GPAMD_EINVAL, what, "the grid spacing must be positive and finite");
    g->off[i] = (int)M; g->coff[i] = (int)cells;
    M += m[i];
    cells += m[i] - 3;
    if (M > SKI_MAX_NODES) return fail(GPAMD_EUNSUPPORTED, what, "the grid has more than 2^24 nodes");
    g->g0[i] = g0[i]; g->h[i] = h[i]; g->m[i] = m[i];
  }
  for (int i = d; i <= SKI_ADD_MAX_DIM; ++i) {
    g->off[i] = (int)M; g->coff[i] = (int)cells;
  }
  g->d = d;
  return 0;
}

template <typename F>
void with_tc(int tc, F&& f) {
  switch (tc) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, SKI_C>{}); break;
  }
}

}  // namespace

extern "C" {

int gpamd_ski_prepare_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, int* keys, void* stream) {
  SkiGrid g;
  int64_t M, cells;
  const int rc = ski_grid("ski_prepare", d, g0, h, m, &g, &M, &cells);
  if (rc) return rc;
  if (!X || !keys) return fail(GPAMD_EINVAL, "ski_prepare: null pointer");
  if (n <= 0) return fail(GPAMD_EINVAL, "ski_prepare: bad shape");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_prepare: the row stride of the points must be >= d");
  SkiPrepArgs a;
  a.X = X; a.ldx = ldx; a.keys = keys; a.n = n; a.g = g;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 255) / 256));
  switch (d) {
    case 1: hipLaunchKernelGGL(ski_prepare_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(ski_prepare_kernel<2>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(ski_prepare_kernel<3>, grid, dim3(256), 0, st, a); break;
  }
  return check_launch("ski_prepare");
}

int gpamd_ski_interp_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm, const float* U,
                         int64_t ldg, int t, float* Out, int64_t ld, void* stream) {
  SkiGrid g;
  int64_t M, cells;
  const int rc = ski_grid("ski_interp", d, g0, h, m, &g, &M, &cells);
  if (rc) return rc;
  if (!X || !U || !Out) return fail(GPAMD_EINVAL, "ski_interp: null pointer");
  if (n <= 0 || t <= 0) return fail(GPAMD_EINVAL, "ski_interp: bad shape");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_interp: the row stride of the points must be >= d");
  if (ldg < M || ld < n) return fail(GPAMD_EINVAL, "ski_interp: leading dimensions must be >= the grid's nodes (U) and n (Out)");
  hipStream_t st = (hipStream_t)stream;
  int c0 = 0;
  while (c0 < t) {
    const int width = group_width(t - c0);
    SkiGatherArgs a;
    a.X = X; a.ldx = ldx; a.perm = perm;
    a.U = U + (int64_t)c0 * ldg; a.ldg = ldg;
    a.Out = Out + (int64_t)c0 * ld; a.ld = ld;
    a.n = n; a.g = g;
    with_d_tc(d, width, [&](auto DD, auto TT) {
      hipLaunchKernelGGL((ski_gather_kernel<DD(), TT()>), dim3((unsigned)((n + SKI_P - 1) / SKI_P)), dim3(SKI_P), 0, st, a);
    });
    const int rl = check_launch("ski_interp");
    if (rl) return rl;
    c0 += width;
  }
  return 0;
}

int gpamd_ski_interp_grad_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                              const float* GA, const float* CA, const float* GB, const float* CB, int64_t ldg, int64_t ldc, int t, float* dX,
                              int64_t lddx, void* stream) {
  SkiGrid g;
  int64_t M, cells;
  const int rc = ski_grid("ski_interp_grad", d, g0, h, m, &g, &M, &cells);
  if (rc) return rc;
  if (!X || !GA || !CA || !dX) return fail(GPAMD_EINVAL, "ski_interp_grad: null pointer");
  if ((GB == nullptr) != (CB == nullptr)) return fail(GPAMD_EINVAL, "ski_interp_grad: null pointer (the second pair is GB and CB together)");
  if (n <= 0 || t <= 0) return fail(GPAMD_EINVAL, "ski_interp_grad: bad shape");
  if (ldx < d || lddx < d) return fail(GPAMD_EINVAL, "ski_interp_grad: the row strides of the points and of dX must be >= d");
  if (ldg < M || ldc < n) return fail(GPAMD_EINVAL, "ski_interp_grad: leading dimensions must be >= the grid's nodes (GA, GB) and n (CA, CB)");
  SkiGradArgs a;
  a.X = X; a.ldx = ldx; a.perm = perm;
  a.GA = GA; a.CA = CA; a.GB = GB; a.CB = CB; a.ldg = ldg; a.ldc = ldc;
  a.dX = dX; a.lddx = lddx; a.n = n; a.t = t; a.g = g;
  const dim3 grid((unsigned)((n + SKI_P - 1) / SKI_P));
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto DD) {
    if (GB) hipLaunchKernelGGL((ski_interp_grad_kernel<DD(), SKI_GC, true>), grid, dim3(SKI_P), 0, st, a);
    else hipLaunchKernelGGL((ski_interp_grad_kernel<DD(), SKI_GC, false>), grid, dim3(SKI_P), 0, st, a);
  };
  switch (d) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    default: launch(std::integral_constant<int, 3>{}); break;
  }
  return check_launch("ski_interp_grad");
}

int64_t gpamd_ski_workspace_floats(int d, int nchunks, int t) {
  if (d < 1 || d > SKI_MAX_DIM || nchunks <= 0 || t <= 0) return 0;
  return (int64_t)nchunks * (1 << (2 * d)) * t;
}

int gpamd_ski_interp_t_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                           const int* cell_start, const int* chunk_off, const int* chunk_begin, const int* chunk_end, int nchunks, const float* V,
                           int64_t ldv, int t, float* U, int64_t ldg, float* workspace, int64_t workspace_floats, void* stream) {
  SkiGrid g;
  int64_t M, cells;
  const int rc = ski_grid("ski_interp_t", d, g0, h, m, &g, &M, &cells);
  if (rc) return rc;
  if (!X || !perm || !cell_start || !V || !U) return fail(GPAMD_EINVAL, "ski_interp_t: null pointer");
  if (n <= 0 || t <= 0 || nchunks < 0) return fail(GPAMD_EINVAL, "ski_interp_t: bad shape");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_interp_t: the row stride of the points must be >= d");
  if (ldg < M || ldv < n) return fail(GPAMD_EINVAL, "ski_interp_t: leading dimensions must be >= n (V) and the grid's nodes (U)");
  if (nchunks > 0) {
    if (!chunk_off || !chunk_begin || !chunk_end || !workspace) return fail(GPAMD_EINVAL, "ski_interp_t: null pointer (chunk lists of the long cells)");
    if (workspace_floats < gpamd_ski_workspace_floats(d, nchunks, t))
      return fail(GPAMD_EWORKSPACE, "ski_interp_t: workspace smaller than gpamd_ski_workspace_floats(d, nchunks, t)");
  }
  hipStream_t st = (hipStream_t)stream;
  int c0 = 0;
  while (c0 < t) {
    const int width = group_width(t - c0);
    SkiScatterArgs a;
    a.X = X; a.ldx = ldx; a.perm = perm; a.cell_start = cell_start;
    a.chunk_off = nchunks > 0 ? chunk_off : nullptr;
    a.chunk_begin = chunk_begin; a.chunk_end = chunk_end;
    a.V = V + (int64_t)c0 * ldv; a.ldv = ldv;
    a.U = U + (int64_t)c0 * ldg; a.ldg = ldg;
    a.H = nchunks > 0 ? workspace + c0 : nullptr; a.hstride = t;
    a.M = (int)M; a.g = g;
    with_d_tc(d, width, [&](auto DD, auto TT) {
      if (nchunks > 0) hipLaunchKernelGGL((ski_heavy_kernel<DD(), TT()>), dim3((unsigned)nchunks), dim3(256), 0, st, a);
      hipLaunchKernelGGL((ski_scatter_kernel<DD(), TT()>), dim3((unsigned)((M + SKI_G - 1) / SKI_G)), dim3(SKI_G), 0, st, a);
    });
    const int rl = check_launch("ski_interp_t");
    if (rl) return rl;
    c0 += width;
  }
  return 0;
}

int gpamd_ski_add_prepare_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, int* keys, void* stream) {
  SkiAddGrid g;
  const int rc = ski_add_grid("ski_add_prepare", d, g0, h, m, &g);
  if (rc) return rc;
  if (!X || !keys) return fail(GPAMD_EINVAL, "ski_add_prepare: null pointer");
  if (n <= 0 || (int64_t)n * d > INT32_MAX) return fail(GPAMD_EINVAL, "ski_add_prepare: bad shape (n >= 1 and d n < 2^31)");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_add_prepare: the row stride of the points must be >= d");
  SkiAddPrepArgs a;
  a.X = X; a.ldx = ldx; a.keys = keys; a.n = n; a.g = g;
  hipLaunchKernelGGL(ski_add_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ski_add_prepare");
}

int gpamd_ski_add_interp_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                             const float* U, int64_t ldg, int t, float* Out, int64_t ld, void* stream) {
  SkiAddGrid g;
  const int rc = ski_add_grid("ski_add_interp", d, g0, h, m, &g);
  if (rc) return rc;
  if (!X || !U || !Out) return fail(GPAMD_EINVAL, "ski_add_interp: null pointer");
  if (n <= 0 || t <= 0) return fail(GPAMD_EINVAL, "ski_add_interp: bad shape");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_add_interp: the row stride of the points must be >= d");
  if (ldg < g.off[d] || ld < n) return fail(GPAMD_EINVAL, "ski_add_interp: leading dimensions must be >= the grid's nodes (U) and n (Out)");
  hipStream_t st = (hipStream_t)stream;
  int c0 = 0;
  while (c0 < t) {
    const int width = group_width(t - c0);
    SkiAddGatherArgs a;
    a.X = X; a.ldx = ldx; a.perm = perm;
    a.U = U + (int64_t)c0 * ldg; a.ldg = ldg;
    a.Out = Out + (int64_t)c0 * ld; a.ld = ld;
    a.n = n; a.g = g;
    with_tc(width, [&](auto TT) {
      hipLaunchKernelGGL((ski_add_gather_kernel<TT()>), dim3((unsigned)((n + SKI_P - 1) / SKI_P)), dim3(SKI_P), 0, st, a);
    });
    const int rl = check_launch("ski_add_interp");
    if (rl) return rl;
    c0 += width;
  }
  return 0;
}

int64_t gpamd_ski_add_workspace_floats(int d, int nchunks, int t) {
  if (d < SKI_ADD_MIN_DIM || d > SKI_ADD_MAX_DIM || nchunks <= 0 || t <= 0) return 0;
  return (int64_t)nchunks * 4 * t;
}

int gpamd_ski_add_interp_t_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                               const int* cell_start, const int* chunk_off, const int* chunk_begin, const int* chunk_end, int nchunks,
                               const float* V, int64_t ldv, int t, float* U, int64_t ldg, float* workspace, int64_t workspace_floats,
                               void* stream) {
  SkiAddGrid g;
  const int rc = ski_add_grid("ski_add_interp_t", d, g0, h, m, &g);
  if (rc) return rc;
  if (!X || !perm || !cell_start || !V || !U) return fail(GPAMD_EINVAL, "ski_add_interp_t: null pointer");
  if (n <= 0 || t <= 0 || nchunks < 0 || (int64_t)n * d > INT32_MAX) return fail(GPAMD_EINVAL, "ski_add_interp_t: bad shape (d n < 2^31)");
  if (ldx < d) return fail(GPAMD_EINVAL, "ski_add_interp_t: the row stride of the points must be >= d");
  if (ldg < g.off[d] || ldv < n) return fail(GPAMD_EINVAL, "ski_add_interp_t: leading dimensions must be >= n (V) and the grid's nodes (U)");
  if (nchunks > 0) {
    if (!chunk_off || !chunk_begin || !chunk_end || !workspace)
      return fail(GPAMD_EINVAL, "ski_add_interp_t: null pointer (chunk lists of the long cells)");
    if (workspace_floats < gpamd_ski_add_workspace_floats(d, nchunks, t))
      return fail(GPAMD_EWORKSPACE, "ski_add_interp_t: workspace smaller than gpamd_ski_add_workspace_floats(d, nchunks, t)");
  }
  hipStream_t st = (hipStream_t)stream;
  const int M = g.off[d];
  int c0 = 0;
  while (c0 < t) {
    const int width = group_width(t - c0);
    SkiAddScatterArgs a;
    a.X = X; a.ldx = ldx; a.perm = perm; a.cell_start = cell_start;
    a.chunk_off = nchunks > 0 ? chunk_off : nullptr;
    a.chunk_begin = chunk_begin; a.chunk_end = chunk_end;
    a.V = V + (int64_t)c0 * ldv; a.ldv = ldv;
    a.U = U + (int64_t)c0 * ldg; a.ldg = ldg;
    a.H = nchunks > 0 ? workspace + c0 : nullptr; a.hstride = t;
    a.n = n; a.M = M; a.g = g;
    with_tc(width, [&](auto TT) {
      if (nchunks > 0) hipLaunchKernelGGL((ski_add_heavy_kernel<TT()>), dim3((unsigned)nchunks), dim3(256), 0, st, a);
      hipLaunchKernelGGL((ski_add_scatter_kernel<TT()>), dim3((unsigned)((M + SKI_G - 1) / SKI_G)), dim3(SKI_G), 0, st, a);
    });
    const int rl = check_launch("ski_add_interp_t");
    if (rl) return rl;
    c0 += width;
  }
  return 0;
}

}  // extern "C"
