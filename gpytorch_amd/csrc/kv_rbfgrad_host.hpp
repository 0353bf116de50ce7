// Host side of the kernels with derivative observations (kv_rbfgrad.hpp, kv_rbfgradgrad.hpp), written once for every radial family F and every
// derivative order O (1: value + gradient, d + 1 components per point; 2: + the d non-mixed second derivatives, 2 d + 1 components, RBF only): the
// split-j plan, the argument checks (all before any launch) and the launches.  extra_rbfgrad.hip, extra_m52grad.hip and extra_rbfgradgrad.hip
// instantiate it and export the C symbols; `who` is the prefix of the error messages, so that a message names the entry point that was called.
#pragma once
#include <type_traits>

#include "host.hpp"
#include "kv_rbfgrad.hpp"
#include "kv_rbfgradgrad.hpp"

namespace gpamd {
namespace rgh {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// split-j plan: units = row blocks x S chunks of whole j tiles; the S whose last round of resident workgroups is fullest, smallest among near-ties
inline void rg_plan(int n, int m, int bm, int bn, int* S, int* jchunk, int* nrb) {
  *nrb = (n + bm - 1) / bm;
  const long slots = (long)num_cus() * 2;
  const int tiles = (m + bn - 1) / bn;
  int smax = m >= 16 * bn ? m / (4 * bn) : tiles;   // small problems: favour parallelism
  if (smax > 48) smax = 48;
  if (smax < 1) smax = 1;
  int best = 1;
  double best_eff = -1.0;
  for (int s = 1; s <= smax; ++s) {
    const int jc = ((m + s - 1) / s + bn - 1) / bn * bn;
    const int se = (m + jc - 1) / jc;
    if (se != s) continue;
    const long units = (long)(*nrb) * se;
    const long rounds = (units + slots - 1) / slots;
    const double last = (double)(m - (long)(se - 1) * jc) / (double)jc;
    const double eff = (double)(*nrb) * ((se - 1) + last) / ((double)rounds * (double)slots);
    if (eff > best_eff + 0.01) {
      best_eff = eff;
      best = s;
    }
  }
  const int jc = ((m + best - 1) / best + bn - 1) / bn * bn;
  *jchunk = jc;
  *S = (m + jc - 1) / jc;
}

// The covariance family whose prepared points a radial family reads
template <int F>
constexpr int prep_kind() {
  return F == KRG_M52 ? GPAMD_MATERN52 : GPAMD_RBF;
}
template <int F>
float rg_invc() {
  return 1.0f / prep_coef<float>(prep_kind<F>(), 0.f);
}

// components per point, and how the messages spell them
template <int O>
constexpr int comps(int d) {
  return O * d + 1;
}
template <int O>
constexpr const char* msg(const char* first, const char* second) {
  return O == 1 ? first : second;
}
// the observation policy of (family, order, d): the one place that maps the host's parameters to the product kernel's template argument
template <int F, int O, int D>
struct rg_obs_of {
  static_assert(O == 1 || (O == 2 && F == KRG_RBF), "second derivatives: the RBF family only");
  using type = std::conditional_t<O == 1, GradObs<F, D>, GradGradObs<D>>;
};
template <int F, int O, int D>
using rg_obs = typename rg_obs_of<F, O, D>::type;

// widest instantiated column count; more columns run as groups, K regenerated per group
template <int F, int O>
constexpr int rg_max_t(int d) {
  return d == 1 ? rg_obs<F, O, 1>::MAX_T : d == 2 ? rg_obs<F, O, 2>::MAX_T : d == 3 ? rg_obs<F, O, 3>::MAX_T : rg_obs<F, O, 4>::MAX_T;
}

template <int F, int O, int D>
const void* rg_kernel_t(int tpad) {
  using OBS = rg_obs<F, O, D>;
  switch (tpad) {
    case 1: return reinterpret_cast<const void*>(kv_gradobs_kernel<OBS, 1>);
    case 2: return reinterpret_cast<const void*>(kv_gradobs_kernel<OBS, 2>);
    default: return reinterpret_cast<const void*>(kv_gradobs_kernel<OBS, OBS::MAX_T>);
  }
}
template <int F, int O>
const void* rg_kernel(int d, int tpad) {
  switch (d) {
    case 1: return rg_kernel_t<F, O, 1>(tpad);
    case 2: return rg_kernel_t<F, O, 2>(tpad);
    case 3: return rg_kernel_t<F, O, 3>(tpad);
    case 4: return rg_kernel_t<F, O, 4>(tpad);
  }
  return nullptr;
}

template <int O = 1>
int plan(const char* who, int n, int m, int d, int t, int64_t ldo, int* S_host, int* jchunk_host, int64_t* workspace_floats_host) {
  if (d < 1 || d > KRG_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, who, "d must be in 1..4");
  if (n <= 0 || m <= 0 || t <= 0 || ldo < (int64_t)n * comps<O>(d))
    return fail(GPAMD_EINVAL, who, msg<O>("bad shape (ldo must be >= n (d + 1))", "bad shape (ldo must be >= n (2 d + 1))"));
  int S, jc, nrb;
  rg_plan(n, m, KRG_BM, KRG_BN, &S, &jc, &nrb);
  if (S_host) *S_host = S;
  if (jchunk_host) *jchunk_host = jc;
  if (workspace_floats_host) *workspace_floats_host = (int64_t)S * t * ldo;
  return 0;
}

template <int F, int O = 1>
int partials(const char* who, const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P,
             int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (d < 1 || d > KRG_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, who, "d must be in 1..4");
  if (!inv_ls || !X1p || !X2p || !Vt || !P) return fail(GPAMD_EINVAL, who, "null pointer");
  if (n <= 0 || m <= 0 || t <= 0 || S <= 0) return fail(GPAMD_EINVAL, who, "bad shape");
  if (ldv < (int64_t)m * comps<O>(d) || ldo < (int64_t)n * comps<O>(d))
    return fail(GPAMD_EINVAL, who, msg<O>("leading dimensions must be >= m (d + 1) and n (d + 1)", "leading dimensions must be >= m (2 d + 1) and n (2 d + 1)"));
  if (!aligned16(X1p) || !aligned16(X2p)) return fail(GPAMD_EINVAL, who, "the prepared points must be 16-byte aligned");
  if (jchunk <= 0 || jchunk % KRG_BN || (int64_t)jchunk * S < m)
    return fail(GPAMD_EINVAL, who, "jchunk * S must cover m and jchunk % 256 == 0 (use the family's plan entry point)");
  hipStream_t st = (hipStream_t)stream;
  const int nrb = (n + KRG_BM - 1) / KRG_BM;
  const int tmax = rg_max_t<F, O>(d);   // (first order: every (family, d) fits at T = 4 without scratch at the same occupancy)
  for (int g0 = 0; g0 < t; g0 += tmax) {
    const int tg = t - g0 < tmax ? t - g0 : tmax;
    KvRgArgs a;
    a.X1 = X1p; a.X2 = X2p;
    a.Vt = Vt + (int64_t)g0 * ldv;
    a.P = P + (int64_t)g0 * ldo;
    a.invl = inv_ls;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jchunk; a.nrb = nrb;
    a.done = done;
    a.invc = rg_invc<F>();
    const void* fn = rg_kernel<F, O>(d, tg <= 1 ? 1 : (tg <= 2 ? 2 : tmax));
    void* kargs[] = {(void*)&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)nrb * (unsigned)S), dim3(256), kargs, 0, st);
    const int rc = check_launch(who);
    if (rc) return rc;
  }
  return 0;
}

inline int64_t grad_workspace_doubles(int n, int m, int d) {
  if (n <= 0 || m <= 0 || d < 1 || d > KRG_MAX_DIM) return 0;
  int S, jc, nrb;
  rg_plan(n, m, KRGG_BM, KRGG_BN, &S, &jc, &nrb);
  return (int64_t)nrb * S * (1 + d);
}

template <int F, int O = 1>
int grad(const char* who, const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl, const float* Rt,
         int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (d < 1 || d > KRG_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, who, "d must be in 1..4");
  if (!inv_ls || !X1p || !X2p || !Lt || !Rt || !out || !workspace) return fail(GPAMD_EINVAL, who, "null pointer");
  if (n <= 0 || m <= 0 || t <= 0) return fail(GPAMD_EINVAL, who, "bad shape");
  if (ldl < (int64_t)n * comps<O>(d) || ldr < (int64_t)m * comps<O>(d))
    return fail(GPAMD_EINVAL, who, msg<O>("leading dimensions must be >= n (d + 1) and m (d + 1)", "leading dimensions must be >= n (2 d + 1) and m (2 d + 1)"));
  if (!aligned16(X1p) || !aligned16(X2p)) return fail(GPAMD_EINVAL, who, "the prepared points must be 16-byte aligned");
  int S, jc, nrb;
  rg_plan(n, m, KRGG_BM, KRGG_BN, &S, &jc, &nrb);
  const int64_t units = (int64_t)nrb * S;
  if (workspace_doubles < units * (1 + d)) return fail(GPAMD_EWORKSPACE, who, "workspace smaller than the family's grad_workspace_doubles(n, m, d)");
  hipStream_t st = (hipStream_t)stream;
  GradRgArgs a;
  a.X1 = X1p; a.X2 = X2p; a.Lt = Lt; a.Rt = Rt; a.invl = inv_ls;
  a.ldl = ldl; a.ldr = ldr;
  a.n = n; a.m = m; a.t = t;
  a.S = S; a.jchunk = jc; a.nrb = nrb;
  a.part = workspace;
  a.invc = rg_invc<F>();
  auto go = [&](auto DD) {
    if constexpr (O == 1) {
      hipLaunchKernelGGL((kv_grad_rbfgrad_kernel<F, DD()>), dim3((unsigned)units), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL(kv_grad_rbfgradgrad_kernel<DD()>, dim3((unsigned)units), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(rbfgrad_finalize_kernel<DD()>, dim3(1), dim3(256), 0, st, (const double*)workspace, (int)units, out);
  };
  switch (d) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 3: go(std::integral_constant<int, 3>{}); break;
    default: go(std::integral_constant<int, 4>{}); break;
  }
  return check_launch(who);
}

}  // namespace rgh
}  // namespace gpamd
