// extern "C" entry points for the fused bilinear-derivative (hyper-parameter gradient) kernel.
#include "host.hpp"
#include "kv_grad.hpp"
#include "kv_directsm.hpp"
#include "kv_grad_ng.hpp"
#include "kv_grad_gibbs.hpp"

using namespace gpamd;

namespace {
constexpr int GRAD_TGROUP = 128;  // probe columns per launch

void grad_plan(int n, int m, int* S, int* jchunk, int* nrb) {
  *nrb = (n + 127) / 128;
  const int slots = num_cus() * 2;
  int smax = m / 256;
  if (smax < 1) smax = 1;
  if (smax > 64) smax = 64;
  int best = 1;
  double best_eff = -1;
  for (int s = 1; s <= smax; ++s) {
    int jc = ((m + s - 1) / s + 63) / 64 * 64;
    int se = (m + jc - 1) / jc;
    long units = (long)(*nrb) * se;
    long rounds = (units + slots - 1) / slots;
    double eff = (double)units / (double)(rounds * slots);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    if (eff >= 0.92) { best = s; break; }
  }
  int jc = ((m + best - 1) / best + 63) / 64 * 64;
  *jchunk = jc;
  *S = (m + jc - 1) / jc;
}

// dp: padded row stride of the prepared points = one of the instantiated dimensions that is a multiple of four (4, 8, 12, 16, 20, 24, 32)
bool grad_dp_ok(int dp) { return dp >= 4 && dp <= KV_MAX_DIM && dp % 4 == 0 && kv_kernel_dims(dp) == dp; }

template <int KIND, int ISO>
void launch_grad(int dp, const GradArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  with_dim(dp, [&](auto DP) {
    if constexpr (DP() % 4 == 0) {
      auto kfn = kv_grad_kernel<KIND, DP(), ISO>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
    }
  });
}
template <int KA, int KB, int DP>
void launch_gradp(const GradArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  auto kfn = kv_gradp_kernel<KA, KB, DP>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
}
template <int KB, int DP>
void launch_grada(const GradArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  auto kfn = kv_grada_kernel<KB, DP>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
}
// Q = Q0 .. Q0 + 3 at compile-time d
template <int DI>
bool launch_grad_sm(int q, const GradSmArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  auto go = [&](auto QQ) {
    if constexpr (ksm_ok(QQ(), DI)) {
      auto kfn = kv_grad_sm_kernel<QQ(), DI>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
    }
  };
  switch (q) {
    case 1: go(std::integral_constant<int, 1>{}); return true;
    case 2: go(std::integral_constant<int, 2>{}); return true;
    case 3: go(std::integral_constant<int, 3>{}); return true;
    case 4: go(std::integral_constant<int, 4>{}); return true;
    case 5: go(std::integral_constant<int, 5>{}); return true;
    case 6: go(std::integral_constant<int, 6>{}); return true;
    case 7: go(std::integral_constant<int, 7>{}); return true;
    case 8: go(std::integral_constant<int, 8>{}); return true;
  }
  return false;
}
// Newton-Girard additive family: base family and d at compile time, the degree cap min(d, 3) or d (ng_cap)
template <int KB, int D>
void launch_grad_ng(int rc, const GradNgArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  auto go = [&](auto RC) {
    auto kfn = kv_grad_ng_kernel<KB, D, RC()>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
  };
  if (rc == D) go(std::integral_constant<int, D>{});
  else go(std::integral_constant<int, ng_cap(D, 1)>{});
}
template <int KB>
void launch_grad_ng_dims(int d, int rc, const GradNgArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  switch (d) {
    case 2: return launch_grad_ng<KB, 2>(rc, a, grid, lds, st);
    case 3: return launch_grad_ng<KB, 3>(rc, a, grid, lds, st);
    case 4: return launch_grad_ng<KB, 4>(rc, a, grid, lds, st);
    case 5: return launch_grad_ng<KB, 5>(rc, a, grid, lds, st);
    case 6: return launch_grad_ng<KB, 6>(rc, a, grid, lds, st);
    case 7: return launch_grad_ng<KB, 7>(rc, a, grid, lds, st);
    case 8: return launch_grad_ng<KB, 8>(rc, a, grid, lds, st);
  }
}
}  // namespace

extern "C" {

int64_t gpamd_kv_grad_workspace_doubles(int n, int m, int t, int dp) {
  int S, jc, nrb;
  if (n <= 0 || m <= 0 || t <= 0) return 0;
  grad_plan(n, m, &S, &jc, &nrb);
  int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  return (int64_t)groups * nrb * S * (1 + dp);
}

int gpamd_kv_grad_f32(int kind, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                      const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                      int64_t workspace_doubles, void* stream) {
  return gpamd_kv_grad_far_f32(kind, X1p, n, X2p, m, dp, Lt, ldl, Rt, ldr, t, iso, out, workspace, workspace_doubles, stream, nullptr, nullptr, nullptr,
                               nullptr, 0.f, nullptr, 0);
}

int64_t gpamd_kv_grad_far_workspace_ints(int n, int m) {
  if (n <= 0 || m <= 0) return 0;
  int S, jc, nrb;
  grad_plan(n, m, &S, &jc, &nrb);
  return (int64_t)nrb * S * (jc / 64 + 1);
}

int gpamd_kv_grad_far_f32(int kind, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                          const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                          int64_t workspace_doubles, void* stream, const float* row_centres, const float* row_radii, const float* tile_centres,
                          const float* tile_radii, float sq_cutoff, int* tile_workspace, int64_t tile_workspace_ints) {
  if (kind < 0 || kind > 3) return fail(GPAMD_EINVAL, "kv_grad: bad arguments");   // (the families with a shape parameter: gpamd_kv_grad_param_far_f32)
  return gpamd_kv_grad_param_far_f32(kind, 0.f, X1p, n, X2p, m, dp, Lt, ldl, Rt, ldr, t, iso, out, workspace, workspace_doubles, stream, row_centres,
                                     row_radii, tile_centres, tile_radii, sq_cutoff, tile_workspace, tile_workspace_ints);
}

int gpamd_kv_grad_param_far_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                                const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                                int64_t workspace_doubles, void* stream, const float* row_centres, const float* row_radii,
                                const float* tile_centres, const float* tile_radii, float sq_cutoff, int* tile_workspace,
                                int64_t tile_workspace_ints) {
  if (!kind_accepted(kind, KINDS_GRAD_PARAM) || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_grad: bad arguments");
  if (const char* bad = kparam_error(kind, kparam)) return fail(GPAMD_EINVAL, "kv_grad", bad);
  if (!grad_dp_ok(dp)) return fail(GPAMD_EUNSUPPORTED, "kv_grad: dp must be one of 4, 8, 12, 16, 20, 24, 32");
  if (kind == GPAMD_PROD) {
    // (this entry point sees the padded stride only: d = D_A + D_B <= 6 means dp is 4 or 8, and the first factor's columns lie inside it)
    if ((dp != 4 && dp != 8) || prod_shape_of((int)kparam).da >= dp) return fail(GPAMD_EINVAL, "kv_grad: the product family takes points prepared with stride 4 or 8 (d = D_A + D_B <= 6)");
    if (iso) return fail(GPAMD_EINVAL, "kv_grad: the product family delivers per-dimension sums only (iso must be 0)");
    if (sq_cutoff > 0.f) return fail(GPAMD_EINVAL, "kv_grad: the product family is not culled (sq_cutoff must be 0)");
  }
  if (kind == GPAMD_ADD) {
    // (the padded stride only: d in 2..8 means dp is 4 or 8; the kernel counts d from the NaN padding of the prepared rows)
    if (dp != 4 && dp != 8) return fail(GPAMD_EINVAL, "kv_grad: the additive family takes points prepared with stride 4 or 8 (d in 2..8)");
    if (iso) return fail(GPAMD_EINVAL, "kv_grad: the additive family delivers per-dimension sums only (iso must be 0)");
    if (sq_cutoff > 0.f) return fail(GPAMD_EINVAL, "kv_grad: the additive family is not culled (sq_cutoff must be 0)");
  }
  int S, jc, nrb;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  const int64_t units = (int64_t)nrb * S;
  if (workspace_doubles < groups * units * (1 + dp)) return fail(GPAMD_EWORKSPACE, "kv_grad: workspace smaller than gpamd_kv_grad_workspace_doubles(n, m, t, dp)");
  hipStream_t st = (hipStream_t)stream;
  const bool cull = sq_cutoff > 0.f;   // far-pair culling (include/gpamd.h gpamd_kv_partials_far_f32): one tile list per unit, shared by the column groups
  if (cull) {
    if (!row_centres || !row_radii || !tile_centres || !tile_radii || !tile_workspace || tile_workspace_ints < units * (jc / 64 + 1))
      return fail(GPAMD_EINVAL, "kv_grad: far-pair culling needs the four bounding-sphere arrays and gpamd_kv_grad_far_workspace_ints ints");
    const CullArgs c = cull_args(row_centres, row_radii, tile_centres, tile_radii, tile_workspace, n, m, dp, 128, 64, nrb, jc, sq_cutoff, nullptr);
    hipLaunchKernelGGL(cull_list_kernel<0>, dim3((unsigned)units), dim3(64), 0, st, c);
  }
  for (int g = 0; g < groups; ++g) {
    const int c0 = g * GRAD_TGROUP;
    const int tg = (t - c0) < GRAD_TGROUP ? (t - c0) : GRAD_TGROUP;
    GradArgs a;
    a.X1 = X1p; a.X2 = X2p;
    a.Lt = Lt + (int64_t)c0 * ldl;
    a.Rt = Rt + (int64_t)c0 * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jc; a.nrb = nrb;
    a.part = workspace + (int64_t)g * units * (1 + dp);
    a.kparam = kparam;
    if (cull) { a.tiles = tile_workspace; a.tpc1 = jc / 64 + 1; }
    const int th = (tg + 1) / 2;
    const size_t lds = ((size_t)4 * 2 * th * 32 + (size_t)4 * 64 * dp) * sizeof(float);
    if (kind == GPAMD_PROD) {
      const ProdShape c = prod_shape_of((int)kparam);
      with_prod_pair(c.ka, c.kb, [&](auto KA, auto KB) {
        if (dp == 4) launch_gradp<KA(), KB(), 4>(a, (unsigned)units, lds, st);
        else launch_gradp<KA(), KB(), 8>(a, (unsigned)units, lds, st);
      });
    } else if (kind == GPAMD_ADD) {
      with_kind<kind_bit(GPAMD_RBF) | kind_bit(GPAMD_MATERN12) | kind_bit(GPAMD_MATERN32) | kind_bit(GPAMD_MATERN52)>((int)kparam, [&](auto KB) {
        if (dp == 4) launch_grada<KB(), 4>(a, (unsigned)units, lds, st);
        else launch_grada<KB(), 8>(a, (unsigned)units, lds, st);
      });
    } else
    with_kind<KINDS_NO_RQ>(kind, [&](auto K) {   // (kind and dp were checked above: a kernel exists)
      if (iso) launch_grad<K(), 1>(dp, a, (unsigned)units, lds, st);
      else launch_grad<K(), 0>(dp, a, (unsigned)units, lds, st);
    });
  }
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, (int)(groups * units), 1 + dp, out);
  return check_launch("kv_grad");
}

int64_t gpamd_kv_sm_grad_workspace_doubles(int n, int m, int t, int q, int d) {
  int S, jc, nrb;
  if (n <= 0 || m <= 0 || t <= 0 || !ksm_ok(q, d)) return 0;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  return (int64_t)groups * nrb * S * (1 + 3 * q * d);
}

int gpamd_kv_sm_grad_f32(const float* block, int q, int d, const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!ksm_ok(q, d)) return fail(GPAMD_EUNSUPPORTED, "kv_sm_grad: (Q, d) outside the native envelope: d in 1..3, Q in 1..8 (d = 1) or 1..4 (d = 2, 3)");
  if (!block) return fail(GPAMD_EINVAL, "kv_sm_grad: null parameter block");
  if (width != ksm_width(q, d)) return fail(GPAMD_EINVAL, "kv_sm_grad: the prepared width must be d + 2 Q d");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_sm_grad: bad arguments");
  int S, jc, nrb;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  const int64_t units = (int64_t)nrb * S;
  const int ng = 1 + 3 * q * d, dp = (width + 3) / 4 * 4;
  if (workspace_doubles < groups * units * ng) return fail(GPAMD_EWORKSPACE, "kv_sm_grad: workspace smaller than gpamd_kv_sm_grad_workspace_doubles(n, m, t, q, d)");
  hipStream_t st = (hipStream_t)stream;
  for (int g = 0; g < groups; ++g) {
    const int c0 = g * GRAD_TGROUP;
    const int tg = (t - c0) < GRAD_TGROUP ? (t - c0) : GRAD_TGROUP;
    GradSmArgs sa;
    GradArgs& a = sa.g;
    a.X1 = X1p; a.X2 = X2p;
    a.Lt = Lt + (int64_t)c0 * ldl;
    a.Rt = Rt + (int64_t)c0 * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jc; a.nrb = nrb;
    a.part = workspace + (int64_t)g * units * ng;
    sa.sm = block;
    const int th = (tg + 1) / 2;
    const size_t lds = ((size_t)4 * 2 * th * 32 + (size_t)4 * 64 * dp) * sizeof(float);
    if (d == 1) launch_grad_sm<1>(q, sa, (unsigned)units, lds, st);
    else if (d == 2) launch_grad_sm<2>(q, sa, (unsigned)units, lds, st);
    else launch_grad_sm<3>(q, sa, (unsigned)units, lds, st);
  }
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, (int)(groups * units), ng, out);
  return check_launch("kv_sm_grad");
}

int64_t gpamd_kv_ng_grad_workspace_doubles(int n, int m, int t, int d, int max_degree) {
  int S, jc, nrb;
  if (n <= 0 || m <= 0 || t <= 0 || !kng_ok(d, max_degree)) return 0;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  return (int64_t)groups * nrb * S * (1 + d + ng_cap(d, max_degree));
}

int gpamd_kv_ng_grad_f32(const float* block, int base, int d, int max_degree, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!kda_dims_ok(d)) return fail(GPAMD_EUNSUPPORTED, "kv_ng_grad: d outside the native envelope 2..8");
  if (!block) return fail(GPAMD_EINVAL, "kv_ng_grad: null weight block");
  if (base < 0 || base > 3) return fail(GPAMD_EINVAL, "kv_ng_grad: base must be the base family's id: 0 (RBF), 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!kng_ok(d, max_degree)) return fail(GPAMD_EINVAL, "kv_ng_grad: max_degree must be in 1..d");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_ng_grad: bad arguments");
  int S, jc, nrb;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  const int64_t units = (int64_t)nrb * S;
  const int rc = ng_cap(d, max_degree), ng = 1 + d + rc, dp = (d + 3) / 4 * 4;
  if (workspace_doubles < groups * units * ng) return fail(GPAMD_EWORKSPACE, "kv_ng_grad: workspace smaller than gpamd_kv_ng_grad_workspace_doubles(n, m, t, d, max_degree)");
  hipStream_t st = (hipStream_t)stream;
  for (int g = 0; g < groups; ++g) {
    const int c0 = g * GRAD_TGROUP;
    const int tg = (t - c0) < GRAD_TGROUP ? (t - c0) : GRAD_TGROUP;
    GradNgArgs na;
    GradArgs& a = na.g;
    a.X1 = X1p; a.X2 = X2p;
    a.Lt = Lt + (int64_t)c0 * ldl;
    a.Rt = Rt + (int64_t)c0 * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jc; a.nrb = nrb;
    a.part = workspace + (int64_t)g * units * ng;
    na.w = block;
    const int th = (tg + 1) / 2;
    const size_t lds = ((size_t)4 * 2 * th * 32 + (size_t)4 * 64 * dp) * sizeof(float);
    with_kind<kind_bit(GPAMD_RBF) | kind_bit(GPAMD_MATERN12) | kind_bit(GPAMD_MATERN32) | kind_bit(GPAMD_MATERN52)>(base, [&](auto KB) {
      launch_grad_ng_dims<KB()>(d, rc, na, (unsigned)units, lds, st);
    });
  }
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, (int)(groups * units), ng, out);
  return check_launch("kv_ng_grad");
}

int64_t gpamd_kv_gibbs_grad_workspace_doubles(int n, int m, int t, int width) {
  int S, jc, nrb;
  if (n <= 0 || m <= 0 || t <= 0 || !kgb_width_ok(width)) return 0;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  return (int64_t)groups * S * ((int64_t)nrb + n);
}

int gpamd_kv_gibbs_grad_f32(const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t,
                            float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!kgb_width_ok(width)) return fail(GPAMD_EUNSUPPORTED, "kv_gibbs_grad: the prepared width must be 4 (up to two input dimensions) or 8 (up to six)");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_gibbs_grad: bad arguments");
  int S, jc, nrb;
  grad_plan(n, m, &S, &jc, &nrb);
  const int groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  const int64_t units = (int64_t)nrb * S;
  if (workspace_doubles < groups * (units + (int64_t)S * n)) return fail(GPAMD_EWORKSPACE, "kv_gibbs_grad: workspace smaller than gpamd_kv_gibbs_grad_workspace_doubles(n, m, t, width)");
  hipStream_t st = (hipStream_t)stream;
  double* rows = workspace + groups * units;   // [groups][S][n] behind the [groups][nrb * S] partial sums of G0
  for (int g = 0; g < groups; ++g) {
    const int c0 = g * GRAD_TGROUP;
    const int tg = (t - c0) < GRAD_TGROUP ? (t - c0) : GRAD_TGROUP;
    GradGibbsArgs ga;
    GradArgs& a = ga.g;
    a.X1 = X1p; a.X2 = X2p;
    a.Lt = Lt + (int64_t)c0 * ldl;
    a.Rt = Rt + (int64_t)c0 * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jc; a.nrb = nrb;
    a.part = workspace + (int64_t)g * units;
    ga.rows = rows + (int64_t)g * S * n;
    const int th = (tg + 1) / 2;
    const size_t lds = ((size_t)4 * 2 * th * 32 + (size_t)4 * 64 * width) * sizeof(float);
    auto go = [&](auto WW) {
      auto kfn = kv_grad_gibbs_kernel<WW()>;
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kfn, dim3((unsigned)units), dim3(256), lds, st, ga);
    };
    if (width == 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
  }
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, (int)(groups * units), 1, out);
  hipLaunchKernelGGL(gibbs_rows_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, groups * S, n, out + 1);
  return check_launch("kv_gibbs_grad");
}

}  // extern "C"
