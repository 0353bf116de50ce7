// Host driver of the device-resident mBCG (cg_kernels.hpp), templated on the scalar type like the kernels.  The entry points
// gpamd_cg_*_f32 (api.hip) and gpamd_cg64_* (extra_f64.hip) forward here with their own name as `what`, so that messages keep naming the
// function that was called; each unit thereby instantiates the kernels of its own scalar type.
#pragma once
#include "cg_kernels.hpp"
#include "host.hpp"

namespace gpamd {

// The float scratch of a solver, in elements: the ONE description behind gpamd_cg_fscratch_elems, gpamd_cg64_fscratch_elems,
// gpamd_cg_layout, gpamd_cg_partials_layout and the pointers of CgState.
struct CgScratch {
  int64_t bnorm, rnorm, rho, stats, alpha_hist, beta_hist, part_a, part_rz, part_rr, total;
};
inline CgScratch cg_scratch(int t, int hist_len) {
  CgScratch L;
  int64_t o = 0;
  L.bnorm = o; o += t;
  L.rnorm = o; o += t;
  L.rho = o; o += 2 * (int64_t)t;
  L.stats = o; o += 4;
  L.alpha_hist = o; o += (int64_t)hist_len * t;
  L.beta_hist = o; o += (int64_t)hist_len * t;
  L.part_a = o; o += (int64_t)t * CG_MAXNB;   // d^T q (and ||b||^2 during init)
  L.part_rz = o; o += (int64_t)t * CG_MAXNB;  // r^T z
  L.part_rr = o; o += (int64_t)t * CG_MAXNB;  // r^T r
  L.total = o;
  return L;
}

template <typename T>
struct CgHandle {   // what the opaque gpamd_cg_t / gpamd_cg64_t derive from
  CgState<T> st;
};

// fills the state of a new solver; false (and the message): bad shape
template <typename T>
bool cg_setup(const char* what, CgState<T>& s, int n, int t, int64_t ld, T* X, T* R, T* D, T* Q, T* Z, T* fscratch, int* iscratch, int hist_len, T eps,
              T stop_updating_after) {
  if (n <= 0 || t <= 0 || ld % 4 || ld < n || hist_len < 0) return fail(GPAMD_EINVAL, what, "bad shape"), false;
  const CgScratch L = cg_scratch(t, hist_len);
  s.X = X; s.R = R; s.D = D; s.Q = Q; s.Z = Z;
  s.ld = ld; s.n = n; s.t = t; s.nb = (int)col_blocks(n, CG_MAXNB);
  s.bnorm = fscratch + L.bnorm;
  s.rnorm = fscratch + L.rnorm;
  s.rho = fscratch + L.rho;
  s.stats = fscratch + L.stats;
  s.alpha_hist = fscratch + L.alpha_hist;
  s.beta_hist = fscratch + L.beta_hist;
  s.part_a = fscratch + L.part_a;
  s.part_rz = fscratch + L.part_rz;
  s.part_rr = fscratch + L.part_rr;
  s.hist_len = hist_len;
  s.zero_rhs = iscratch;
  s.converged = iscratch + t;
  s.done = iscratch + 2 * t;
  s.eps = eps;
  s.stop_updating_after = stop_updating_after;
  return true;
}

// ---- the steps: launches only.  The row-sharded entry points run one step each (the host all-reduces the partial sums between them); the
// un-sharded init / begin / update_d are compositions of the same steps.
template <typename T>
dim3 cg_grid(const CgState<T>& s) { return dim3(s.nb, s.t); }

template <typename T>
void cg_step_init_norms(const CgState<T>& s, const T* B, int64_t ldb, hipStream_t st) {
  (void)hipMemsetAsync(s.done, 0, 2 * sizeof(int), st);
  hipLaunchKernelGGL((coldot_kernel<T>), cg_grid(s), dim3(256), 0, st, B, B, ldb, s.n, s.part_a, (const int*)nullptr);
}
template <typename T>
void cg_step_init_apply(const CgState<T>& s, const T* B, int64_t ldb, int copy_d, hipStream_t st) {
  hipLaunchKernelGGL((cg_init_kernel<T>), cg_grid(s), dim3(256), 0, st, s, B, ldb, copy_d);
}
template <typename T>
void cg_step_begin_apply(const CgState<T>& s, hipStream_t st) {
  hipLaunchKernelGGL((cg_begin_kernel<T>), dim3(s.t), dim3(256), 0, st, s);
}
// done: the solver's done word (a finished solve skips the work) or nullptr (before the first iteration)
template <typename T>
void cg_step_dot_rz(const CgState<T>& s, const int* done, hipStream_t st) {
  hipLaunchKernelGGL((coldot_kernel<T>), cg_grid(s), dim3(256), 0, st, (const T*)s.R, (const T*)s.Z, s.ld, s.n, s.part_rz, done);
}
template <typename T>
void cg_step_update_d_apply(const CgState<T>& s, int k, hipStream_t st) {
  hipLaunchKernelGGL((cg_update_d_kernel<T>), cg_grid(s), dim3(256), 0, st, s, k);
  hipLaunchKernelGGL((cg_stats_kernel<T>), dim3(1), dim3(256), 0, st, s);
}

// ---- the entry points
template <typename T>
int cg_init_norms(const char* what, CgHandle<T>* h, const T* B, int64_t ldb, void* stream) {
  if (!h || ldb % 4) return fail(GPAMD_EINVAL, what, "bad arguments");
  cg_step_init_norms(h->st, B, ldb, (hipStream_t)stream);
  return check_launch(what);
}
template <typename T>
int cg_init_apply(const char* what, CgHandle<T>* h, const T* B, int64_t ldb, int copy_d, void* stream) {
  if (!h || ldb % 4) return fail(GPAMD_EINVAL, what, "bad arguments");
  cg_step_init_apply(h->st, B, ldb, copy_d ? 1 : 0, (hipStream_t)stream);
  return check_launch(what);
}
template <typename T>
int cg_begin_apply(const char* what, CgHandle<T>* h, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  cg_step_begin_apply(h->st, (hipStream_t)stream);
  return check_launch(what);
}
template <typename T>
int cg_dot_rz(const char* what, CgHandle<T>* h, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  cg_step_dot_rz(h->st, h->st.done, (hipStream_t)stream);
  return check_launch(what);
}
template <typename T>
int cg_update_d_apply(const char* what, CgHandle<T>* h, int k, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  cg_step_update_d_apply(h->st, k, (hipStream_t)stream);
  return check_launch(what);
}

template <typename T>
int cg_init(const char* what, CgHandle<T>* h, const T* B, int64_t ldb, int have_precond, void* stream) {
  if (!h || ldb % 4) return fail(GPAMD_EINVAL, what, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  cg_step_init_norms(h->st, B, ldb, st);
  cg_step_init_apply(h->st, B, ldb, have_precond ? 0 : 1, st);
  if (!have_precond) cg_step_begin_apply(h->st, st);
  return check_launch(what);
}
template <typename T>
int cg_begin(const char* what, CgHandle<T>* h, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  cg_step_dot_rz(h->st, (const int*)nullptr, (hipStream_t)stream);
  cg_step_begin_apply(h->st, (hipStream_t)stream);
  return check_launch(what);
}
template <typename T>
int cg_update_d(const char* what, CgHandle<T>* h, int k, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  if (h->st.Z != h->st.R) cg_step_dot_rz(h->st, h->st.done, (hipStream_t)stream);
  cg_step_update_d_apply(h->st, k, (hipStream_t)stream);
  return check_launch(what);
}

template <typename T>
int cg_reduce_q(const char* what, CgHandle<T>* h, const T* P, int S, int64_t ldp, const T* scale, const T* dscale, const T* dvec, void* stream) {
  if (!h || S <= 0 || ldp % 4) return fail(GPAMD_EINVAL, what, "bad arguments");
  const CgState<T>& s = h->st;
  hipLaunchKernelGGL((kv_reduce_kernel<T, true>), cg_grid(s), dim3(256), 0, (hipStream_t)stream, P, S, (int64_t)s.t * ldp, ldp, scale, dscale, dvec,
                     s.D, s.ld, s.Q, s.ld, s.n, s.part_a, s.done);
  return check_launch(what);
}
template <typename T>
int cg_update_xr(const char* what, CgHandle<T>* h, int k, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  hipLaunchKernelGGL((cg_update_xr_kernel<T>), cg_grid(h->st), dim3(256), 0, (hipStream_t)stream, h->st, k, h->st.Z == h->st.R ? 1 : 0);
  return check_launch(what);
}
template <typename T>
int cg_stop(const char* what, CgHandle<T>* h, int k, int min_iter, int tridiag_floor, T tol, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  hipLaunchKernelGGL((cg_stop_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, h->st, k, min_iter, tridiag_floor, tol);
  return check_launch(what);
}
template <typename T>
int cg_finish(const char* what, CgHandle<T>* h, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, what, "null handle");
  hipLaunchKernelGGL((cg_finish_kernel<T>), cg_grid(h->st), dim3(256), 0, (hipStream_t)stream, h->st);
  return check_launch(what);
}

}  // namespace gpamd
