// extern "C" entry points for the fused bilinear-derivative (hyper-parameter gradient) kernel.
#include "host.hpp"
#include "kv_grad.hpp"
#include "kv_directsm.hpp"
#include "kv_grad_ng.hpp"
#include "kv_grad_gibbs.hpp"
#include "kv_grad_ps.hpp"
#include "kv_grad_ham.hpp"

using namespace gpamd;

namespace {
constexpr int GRAD_TGROUP = 128;  // probe columns per launch

// The launch plan of kv_grad_tile: nrb row blocks of 128 x S j chunks of jc points (a multiple of 64) = `units` blocks per column group
struct GradPlan {
  int S, jc, nrb, groups;
  int64_t units;                                          // per column group
  int64_t all_units() const { return groups * units; }    // partial-sum records of one call
};

GradPlan grad_plan(int n, int m, int t) {
  GradPlan p;
  p.nrb = (n + 127) / 128;
  const int slots = num_cus() * 2;
  int smax = m / 256;
  if (smax < 1) smax = 1;
  if (smax > 64) smax = 64;
  int best = 1;
  double best_eff = -1;
  for (int s = 1; s <= smax; ++s) {
    int jc = ((m + s - 1) / s + 63) / 64 * 64;
    int se = (m + jc - 1) / jc;
    long units = (long)p.nrb * se;
    long rounds = (units + slots - 1) / slots;
    double eff = (double)units / (double)(rounds * slots);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    if (eff >= 0.92) { best = s; break; }
  }
  p.jc = ((m + best - 1) / best + 63) / 64 * 64;
  p.S = (m + p.jc - 1) / p.jc;
  p.groups = (t + GRAD_TGROUP - 1) / GRAD_TGROUP;
  p.units = (int64_t)p.nrb * p.S;
  return p;
}

// dp: padded row stride of the prepared points = one of the instantiated dimensions that is a multiple of four (4, 8, 12, 16, 20, 24, 32)
bool grad_dp_ok(int dp) { return dp >= 4 && dp <= KV_MAX_DIM && dp % 4 == 0 && kv_kernel_dims(dp) == dp; }

// One block of 256 threads per unit with `lds` bytes of dynamic LDS
template <typename K, typename A>
void launch_lds(K kfn, unsigned grid, size_t lds, hipStream_t st, const A& a) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
}

// The column-group loop of every entry point below: `base` holds what the groups share (clouds, vectors, sizes, kparam, tile list); per group of up to
// GRAD_TGROUP columns launch(a, g, grid, lds) picks and launches the family's kernel on rows of stride dp; then the groups * units partial records of
// nsums sums each (at the head of the workspace) are summed into out
template <typename L>
void grad_run(const GradPlan& p, GradArgs base, int dp, int nsums, double* workspace, float* out, hipStream_t st, L&& launch) {
  const float *Lt = base.Lt, *Rt = base.Rt;
  const int t = base.t;
  base.S = p.S; base.jchunk = p.jc; base.nrb = p.nrb;
  for (int g = 0; g < p.groups; ++g) {
    const int c0 = g * GRAD_TGROUP;
    GradArgs a = base;
    a.Lt = Lt + (int64_t)c0 * a.ldl;
    a.Rt = Rt + (int64_t)c0 * a.ldr;
    a.t = (t - c0) < GRAD_TGROUP ? (t - c0) : GRAD_TGROUP;
    a.part = workspace + (int64_t)g * p.units * nsums;
    const int th = (a.t + 1) / 2;
    const size_t lds = ((size_t)4 * 2 * th * 32 + (size_t)4 * 64 * dp) * sizeof(float);
    launch(a, g, (unsigned)p.units, lds);
  }
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, (int)p.all_units(), nsums, out);
}

GradArgs grad_base(const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t) {
  GradArgs a;
  a.X1 = X1p; a.X2 = X2p;
  a.Lt = Lt; a.Rt = Rt;
  a.ldl = ldl; a.ldr = ldr;
  a.n = n; a.m = m; a.t = t;
  return a;
}

// Integer dispatch in the manner of with_dim (host.hpp): calls f(std::integral_constant<int, V>) for the listed V == v; false when none is
template <typename F, int... V>
bool with_int(int v, std::integer_sequence<int, V...>, F&& f) {
  return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
constexpr unsigned KINDS_BASE = kind_bit(GPAMD_RBF) | kind_bit(GPAMD_MATERN12) | kind_bit(GPAMD_MATERN32) | kind_bit(GPAMD_MATERN52);   // base families of the additive kernels
constexpr unsigned KINDS_MATERN = KINDS_BASE & ~kind_bit(GPAMD_RBF);   // ... and of the product-structure kernels
}  // namespace

extern "C" {

int64_t gpamd_kv_grad_workspace_doubles(int n, int m, int t, int dp) {
  if (n <= 0 || m <= 0 || t <= 0) return 0;
  return grad_plan(n, m, t).all_units() * (1 + dp);
}

int gpamd_kv_grad_f32(int kind, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                      const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                      int64_t workspace_doubles, void* stream) {
  return gpamd_kv_grad_far_f32(kind, X1p, n, X2p, m, dp, Lt, ldl, Rt, ldr, t, iso, out, workspace, workspace_doubles, stream, nullptr, nullptr, nullptr,
                               nullptr, 0.f, nullptr, 0);
}

int64_t gpamd_kv_grad_far_workspace_ints(int n, int m) {
  if (n <= 0 || m <= 0) return 0;
  const GradPlan p = grad_plan(n, m, 1);
  return p.units * (p.jc / 64 + 1);
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
  const GradPlan p = grad_plan(n, m, t);
  if (workspace_doubles < p.all_units() * (1 + dp)) return fail(GPAMD_EWORKSPACE, "kv_grad: workspace smaller than gpamd_kv_grad_workspace_doubles(n, m, t, dp)");
  hipStream_t st = (hipStream_t)stream;
  GradArgs base = grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t);
  base.kparam = kparam;
  if (sq_cutoff > 0.f) {   // far-pair culling (include/gpamd.h gpamd_kv_partials_far_f32): one tile list per unit, shared by the column groups
    if (!row_centres || !row_radii || !tile_centres || !tile_radii || !tile_workspace || tile_workspace_ints < p.units * (p.jc / 64 + 1))
      return fail(GPAMD_EINVAL, "kv_grad: far-pair culling needs the four bounding-sphere arrays and gpamd_kv_grad_far_workspace_ints ints");
    const CullArgs c = cull_args(row_centres, row_radii, tile_centres, tile_radii, tile_workspace, n, m, dp, 128, 64, p.nrb, p.jc, sq_cutoff, nullptr);
    hipLaunchKernelGGL(cull_list_kernel<0>, dim3((unsigned)p.units), dim3(64), 0, st, c);
    base.tiles = tile_workspace;
    base.tpc1 = p.jc / 64 + 1;
  }
  grad_run(p, base, dp, 1 + dp, workspace, out, st, [&](const GradArgs& a, int, unsigned grid, size_t lds) {
    if (kind == GPAMD_PROD) {
      const ProdShape c = prod_shape_of((int)kparam);
      with_prod_pair(c.ka, c.kb, [&](auto KA, auto KB) {
        with_int(dp, std::integer_sequence<int, 4, 8>{}, [&](auto DP) { launch_lds(kv_gradp_kernel<KA(), KB(), DP()>, grid, lds, st, a); });
      });
    } else if (kind == GPAMD_ADD) {
      with_kind<KINDS_BASE>((int)kparam, [&](auto KB) {
        with_int(dp, std::integer_sequence<int, 4, 8>{}, [&](auto DP) { launch_lds(kv_grada_kernel<KB(), DP()>, grid, lds, st, a); });
      });
    } else {
      with_kind<KINDS_NO_RQ>(kind, [&](auto K) {   // (kind and dp were checked above: a kernel exists)
        with_dim(dp, [&](auto DP) {
          if constexpr (DP() % 4 == 0) {
            if (iso) launch_lds(kv_grad_kernel<K(), DP(), 1>, grid, lds, st, a);
            else launch_lds(kv_grad_kernel<K(), DP(), 0>, grid, lds, st, a);
          }
        });
      });
    }
  });
  return check_launch("kv_grad");
}

int64_t gpamd_kv_sm_grad_workspace_doubles(int n, int m, int t, int q, int d) {
  if (n <= 0 || m <= 0 || t <= 0 || !ksm_ok(q, d)) return 0;
  return grad_plan(n, m, t).all_units() * (1 + 3 * q * d);
}

int gpamd_kv_sm_grad_f32(const float* block, int q, int d, const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!ksm_ok(q, d)) return fail(GPAMD_EUNSUPPORTED, "kv_sm_grad: (Q, d) outside the native envelope: d in 1..3, Q in 1..8 (d = 1) or 1..4 (d = 2, 3)");
  if (!block) return fail(GPAMD_EINVAL, "kv_sm_grad: null parameter block");
  if (width != ksm_width(q, d)) return fail(GPAMD_EINVAL, "kv_sm_grad: the prepared width must be d + 2 Q d");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_sm_grad: bad arguments");
  const GradPlan p = grad_plan(n, m, t);
  const int ng = 1 + 3 * q * d, dp = (width + 3) / 4 * 4;
  if (workspace_doubles < p.all_units() * ng) return fail(GPAMD_EWORKSPACE, "kv_sm_grad: workspace smaller than gpamd_kv_sm_grad_workspace_doubles(n, m, t, q, d)");
  hipStream_t st = (hipStream_t)stream;
  grad_run(p, grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t), dp, ng, workspace, out, st, [&](const GradArgs& a, int, unsigned grid, size_t lds) {
    const GradSmArgs sa{a, block};
    with_int(d, std::integer_sequence<int, 1, 2, 3>{}, [&](auto DI) {
      with_int(q, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>{}, [&](auto Q) {
        if constexpr (ksm_ok(Q(), DI())) launch_lds(kv_grad_sm_kernel<Q(), DI()>, grid, lds, st, sa);
      });
    });
  });
  return check_launch("kv_sm_grad");
}

int64_t gpamd_kv_ng_grad_workspace_doubles(int n, int m, int t, int d, int max_degree) {
  if (n <= 0 || m <= 0 || t <= 0 || !kng_ok(d, max_degree)) return 0;
  return grad_plan(n, m, t).all_units() * (1 + d + ng_cap(d, max_degree));
}

int gpamd_kv_ng_grad_f32(const float* block, int base, int d, int max_degree, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!kda_dims_ok(d)) return fail(GPAMD_EUNSUPPORTED, "kv_ng_grad: d outside the native envelope 2..8");
  if (!block) return fail(GPAMD_EINVAL, "kv_ng_grad: null weight block");
  if (base < 0 || base > 3) return fail(GPAMD_EINVAL, "kv_ng_grad: base must be the base family's id: 0 (RBF), 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!kng_ok(d, max_degree)) return fail(GPAMD_EINVAL, "kv_ng_grad: max_degree must be in 1..d");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_ng_grad: bad arguments");
  const GradPlan p = grad_plan(n, m, t);
  const int rc = ng_cap(d, max_degree), ng = 1 + d + rc, dp = (d + 3) / 4 * 4;
  if (workspace_doubles < p.all_units() * ng) return fail(GPAMD_EWORKSPACE, "kv_ng_grad: workspace smaller than gpamd_kv_ng_grad_workspace_doubles(n, m, t, d, max_degree)");
  hipStream_t st = (hipStream_t)stream;
  grad_run(p, grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t), dp, ng, workspace, out, st, [&](const GradArgs& a, int, unsigned grid, size_t lds) {
    const GradNgArgs na{a, block};
    // base family and d at compile time, the degree cap min(d, 3) or d (ng_cap)
    with_kind<KINDS_BASE>(base, [&](auto KB) {
      with_int(d, std::integer_sequence<int, 2, 3, 4, 5, 6, 7, 8>{}, [&](auto D) {
        if (rc == D()) launch_lds(kv_grad_ng_kernel<KB(), D(), D()>, grid, lds, st, na);
        else launch_lds(kv_grad_ng_kernel<KB(), D(), ng_cap(D(), 1)>, grid, lds, st, na);
      });
    });
  });
  return check_launch("kv_ng_grad");
}

int64_t gpamd_kv_ps_grad_workspace_doubles(int n, int m, int t, int d) {
  if (n <= 0 || m <= 0 || t <= 0 || !kda_dims_ok(d)) return 0;
  return grad_plan(n, m, t).all_units() * (1 + d);
}

int gpamd_kv_ps_grad_f32(int base, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t,
                         float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!kda_dims_ok(d)) return fail(GPAMD_EUNSUPPORTED, "kv_ps_grad: d outside the native envelope 2..8");
  if (base == GPAMD_RBF) return fail(GPAMD_EINVAL, "kv_ps_grad: a product of one-dimensional RBFs IS the RBF family with per-dimension lengthscales (GPAMD_RBF): base must be 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!kps_base_ok(base)) return fail(GPAMD_EINVAL, "kv_ps_grad: base must be the base family's id: 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_ps_grad: bad arguments");
  const GradPlan p = grad_plan(n, m, t);
  const int ng = 1 + d, dp = (d + 3) / 4 * 4;
  if (workspace_doubles < p.all_units() * ng) return fail(GPAMD_EWORKSPACE, "kv_ps_grad: workspace smaller than gpamd_kv_ps_grad_workspace_doubles(n, m, t, d)");
  hipStream_t st = (hipStream_t)stream;
  grad_run(p, grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t), dp, ng, workspace, out, st, [&](const GradArgs& a, int, unsigned grid, size_t lds) {
    with_kind<KINDS_MATERN>(base, [&](auto KB) {   // base family and d at compile time
      with_int(d, std::integer_sequence<int, 2, 3, 4, 5, 6, 7, 8>{}, [&](auto D) { launch_lds(kv_grad_ps_kernel<KB(), D()>, grid, lds, st, a); });
    });
  });
  return check_launch("kv_ps_grad");
}

int64_t gpamd_kv_hamming_grad_workspace_doubles(int n, int m, int t, int width) {
  if (n <= 0 || m <= 0 || t <= 0 || !khm_width_ok(width)) return 0;
  return grad_plan(n, m, t).all_units() * 3;
}

int gpamd_kv_hamming_grad_f32(int width, float inv_alpha, float beta, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                              const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!khm_width_ok(width)) return fail(GPAMD_EUNSUPPORTED, "kv_hamming_grad: the prepared width must be 4, 8, 16 or 32 dwords (up to 16, 32, 64, 128 positions)");
  if (!khm_param_ok(inv_alpha) || !khm_param_ok(beta)) return fail(GPAMD_EINVAL, "kv_hamming_grad: 1 / alpha and beta must be positive and finite");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_hamming_grad: bad arguments");
  const GradPlan p = grad_plan(n, m, t);
  if (workspace_doubles < p.all_units() * 3) return fail(GPAMD_EWORKSPACE, "kv_hamming_grad: workspace smaller than gpamd_kv_hamming_grad_workspace_doubles(n, m, t, width)");
  hipStream_t st = (hipStream_t)stream;
  grad_run(p, grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t), width, 3, workspace, out, st, [&](const GradArgs& a, int, unsigned grid, size_t lds) {
    const GradHamArgs ha{a, inv_alpha, beta};
    with_int(width, std::integer_sequence<int, 4, 8, 16, 32>{}, [&](auto W) { launch_lds(kv_grad_ham_kernel<W()>, grid, lds, st, ha); });
  });
  return check_launch("kv_hamming_grad");
}

int64_t gpamd_kv_gibbs_grad_workspace_doubles(int n, int m, int t, int width) {
  if (n <= 0 || m <= 0 || t <= 0 || !kgb_width_ok(width)) return 0;
  const GradPlan p = grad_plan(n, m, t);
  return p.all_units() + (int64_t)p.groups * p.S * n;
}

int gpamd_kv_gibbs_grad_f32(const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t,
                            float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  if (!kgb_width_ok(width)) return fail(GPAMD_EUNSUPPORTED, "kv_gibbs_grad: the prepared width must be 4 (up to two input dimensions) or 8 (up to six)");
  if (!X1p || !X2p || !Lt || !Rt || !out || !workspace || n <= 0 || m <= 0 || t <= 0 || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_gibbs_grad: bad arguments");
  const GradPlan p = grad_plan(n, m, t);
  if (workspace_doubles < p.all_units() + (int64_t)p.groups * p.S * n) return fail(GPAMD_EWORKSPACE, "kv_gibbs_grad: workspace smaller than gpamd_kv_gibbs_grad_workspace_doubles(n, m, t, width)");
  hipStream_t st = (hipStream_t)stream;
  double* rows = workspace + p.all_units();   // [groups][S][n] behind the [groups][nrb * S] partial sums of G0
  grad_run(p, grad_base(X1p, n, X2p, m, Lt, ldl, Rt, ldr, t), width, 1, workspace, out, st, [&](const GradArgs& a, int g, unsigned grid, size_t lds) {
    const GradGibbsArgs ga{a, rows + (int64_t)g * p.S * n};
    with_int(width, std::integer_sequence<int, 4, 8>{}, [&](auto W) { launch_lds(kv_grad_gibbs_kernel<W()>, grid, lds, st, ga); });
  });
  hipLaunchKernelGGL(gibbs_rows_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, p.groups * p.S, n, out + 1);
  return check_launch("kv_gibbs_grad");
}

}  // extern "C"
