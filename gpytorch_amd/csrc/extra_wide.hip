// Wide inputs, 33 .. 512 dimensions (kv_wide.hpp): the fused product kernels for RBF and Matern 3/2, 5/2 with CT = 1, 2 column tiles, with and without the
// extra VALU column, NI = 1, 2 row tiles per wave -- the number of dimensions is a run-time chunk count --, the split pre-pass of a prepared cloud, and
// the entry points gpamd_wide_split_f32, gpamd_kv_wide_plan, gpamd_kv_wide_partials_f32; the derivative kernels of the same clouds (kv_wide_grad.hpp), their
// transposed-image pre-pass and gpamd_wide_split_t_f32, gpamd_kv_wide_grad_workspace_doubles, gpamd_kv_wide_grad_f32; the direct-difference product kernels
// of the clouds outside the norm rule and of Matern 1/2 (kv_wide_direct.hpp) and gpamd_kv_wide_direct_plan, gpamd_kv_wide_direct_partials_f32; their
// derivative kernels (kv_wide_direct_grad.hpp) and gpamd_kv_wide_direct_grad_workspace_doubles, gpamd_kv_wide_direct_grad_f32.
#include "host.hpp"
#include "kv_wide.hpp"
#include "kv_wide_direct.hpp"
#include "kv_wide_direct_grad.hpp"
#include "kv_wide_grad.hpp"

using namespace gpamd;

namespace {

template <int KIND, int CT>
const void* wide_ptr_ex(int ex) {
  return ex ? reinterpret_cast<const void*>(&kv_wide_kernel<KIND, CT, KW_NI, 1>) : reinterpret_cast<const void*>(&kv_wide_kernel<KIND, CT, KW_NI, 0>);
}
template <int KIND>
const void* wide_ptr_kind(int ct, int ex) {
  if (ct == 1) return wide_ptr_ex<KIND, 1>(ex);
  if (ct == 2) return wide_ptr_ex<KIND, 2>(ex);
  return nullptr;
}
const void* wide_ptr(int kind, int ct, int ex) {
  switch (kind) {
    case GPAMD_RBF: return wide_ptr_kind<KIND_RBF>(ct, ex);
    case GPAMD_MATERN32: return wide_ptr_kind<KIND_MATERN32>(ct, ex);
    case GPAMD_MATERN52: return wide_ptr_kind<KIND_MATERN52>(ct, ex);
  }
  return nullptr;
}

bool wide_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool wide_kind_ok(int kind) { return kind == GPAMD_RBF || kind == GPAMD_MATERN32 || kind == GPAMD_MATERN52; }
constexpr const char* WIDE_KINDS = "kv_wide: the wide kernels take RBF and Matern 3/2, 5/2 only";
constexpr const char* WIDE_DIMS = "kv_wide: d outside the native envelope 33..512";

// launch groups of <= 64 (+ 1) columns, as the split-operand kernels of api.hip take them: columns of group g0, its extra column, its column tiles
struct WideGroup { int tg, ex, ct; };
WideGroup wide_group(int t, int g0) {
  WideGroup g;
  g.tg = (t - g0 <= KGH_GROUP + 1) ? t - g0 : KGH_GROUP;
  g.ex = (g.tg % 32 == 1 && g.tg > 1) ? 1 : 0;
  g.ct = (g.tg - g.ex + 31) / 32;
  return g;
}

// Behind the S slabs: column maxima | column multipliers (32 ct + 1 slots per group) | the two f16 planes of every group.  Offsets in floats, multiples of 4
struct WideLayout {
  int64_t base, colmax, colmul, planes, total, ldh;
  int slots;
};
WideLayout wide_layout(int m, int t, int S, int64_t ldo) {
  WideLayout L{};
  L.base = ((int64_t)S * t * ldo + 3) / 4 * 4;
  L.ldh = ((int64_t)m + KGH_BN - 1) / KGH_BN * KGH_BN;
  int64_t rows = 0;
  int slots = 0;
  for (int g0 = 0; g0 < t;) {
    const WideGroup g = wide_group(t, g0);
    rows += 32 * g.ct;
    slots += 32 * g.ct + 1;
    g0 += g.tg;
  }
  L.slots = (slots + 3) / 4 * 4;
  L.colmax = 0;
  L.colmul = L.slots;
  L.planes = 2 * (int64_t)L.slots;
  L.total = L.planes + rows * L.ldh;   // two f16 planes of `rows` rows = rows x ldh floats
  return L;
}

// ---- the direct-difference product (kv_wide_direct.hpp): sixteen instantiations, NI = KWD_NI
template <int KIND, int CT>
const void* wide_direct_ptr_ex(int ex) {
  return ex ? reinterpret_cast<const void*>(&kv_wide_direct_kernel<KIND, CT, KWD_NI, 1>) : reinterpret_cast<const void*>(&kv_wide_direct_kernel<KIND, CT, KWD_NI, 0>);
}
template <int KIND>
const void* wide_direct_ptr_kind(int ct, int ex) {
  if (ct == 1) return wide_direct_ptr_ex<KIND, 1>(ex);
  if (ct == 2) return wide_direct_ptr_ex<KIND, 2>(ex);
  return nullptr;
}
const void* wide_direct_ptr(int kind, int ct, int ex) {
  switch (kind) {
    case GPAMD_RBF: return wide_direct_ptr_kind<KIND_RBF>(ct, ex);
    case GPAMD_MATERN12: return wide_direct_ptr_kind<KIND_MATERN12>(ct, ex);
    case GPAMD_MATERN32: return wide_direct_ptr_kind<KIND_MATERN32>(ct, ex);
    case GPAMD_MATERN52: return wide_direct_ptr_kind<KIND_MATERN52>(ct, ex);
  }
  return nullptr;
}
bool wide_direct_kind_ok(int kind) { return wide_kind_ok(kind) || kind == GPAMD_MATERN12; }
constexpr const char* WIDE_DIRECT_KINDS = "kv_wide_direct: the wide direct-difference kernels take RBF and Matern 1/2, 3/2, 5/2 only";
constexpr const char* WIDE_DIRECT_DIMS = "kv_wide_direct: d outside the native envelope 33..512";
// Split-j plan: enough (row block, slab) units for every compute unit to hold the workgroups its registers admit (kwd_waves per SIMD: two workgroups at
// NI = 1, one at NI = 2, on each of 256 compute units), slabs of whole 128-row tiles
void wide_direct_split(int n, int m, int* S_out, int* jchunk_out) {
  const int nrb = (n + kgh_bm(KWD_NI) - 1) / kgh_bm(KWD_NI), tiles = kw_tiles(m);
  const int target = 256 * kwd_waves(KWD_NI);
  int S = (target + nrb - 1) / nrb;
  S = S < 1 ? 1 : (S > tiles ? tiles : S);
  const int per = (tiles + S - 1) / S;
  *S_out = (tiles + per - 1) / per;
  *jchunk_out = per * KW_TILE;
}

// ---- the derivative kernel (kv_wide_grad.hpp).  Resource usage of the six instantiations: the build's remarks (no scratch; two waves per SIMD)
template <int KIND>
const void* wide_grad_ptr_kind(int mode) {
  return mode ? reinterpret_cast<const void*>(&kv_wide_grad_kernel<KIND, 1>) : reinterpret_cast<const void*>(&kv_wide_grad_kernel<KIND, 0>);
}
const void* wide_grad_ptr(int kind, int mode) {
  switch (kind) {
    case GPAMD_RBF: return wide_grad_ptr_kind<KIND_RBF>(mode);
    case GPAMD_MATERN32: return wide_grad_ptr_kind<KIND_MATERN32>(mode);
    case GPAMD_MATERN52: return wide_grad_ptr_kind<KIND_MATERN52>(mode);
  }
  return nullptr;
}

// Split-j plan and workspace of the derivative: enough (row block, slab, dimension block) units for two workgroups on each of 256 compute units,
// slabs of whole 128-row tiles.  Offsets in doubles: partial sums [npass][nrb S][pstride] | sc u [npass][S][n][dq] floats | sc rs [npass][S][n] floats
constexpr int KWG_TARGET_UNITS = 512;
struct WideGradLayout {
  int nrb, ndb, S, jchunk, npass, pstride, dq;
  int64_t u, rs, total;
};
WideGradLayout wide_grad_layout(int n, int m, int d, int t, int mode) {
  WideGradLayout L{};
  L.nrb = kw_tiles(n);
  L.ndb = mode ? kwg_dblocks(d) : 1;
  L.dq = KWG_DB * kwg_dblocks(d);
  const int tiles = kw_tiles(m);
  int S = (KWG_TARGET_UNITS + L.nrb * L.ndb - 1) / (L.nrb * L.ndb);
  S = S < 1 ? 1 : (S > tiles ? tiles : S);
  const int per = (tiles + S - 1) / S;
  L.S = (tiles + per - 1) / per;
  L.jchunk = per * KW_TILE;
  L.npass = (t + KWG_MAXT - 1) / KWG_MAXT;
  L.pstride = mode ? 1 + L.dq : 2;
  const int64_t parts = ((int64_t)L.npass * L.nrb * L.S * L.pstride + 1) / 2 * 2;
  L.u = parts;
  const int64_t uf = mode == 3 ? (int64_t)L.npass * L.S * n * L.dq : 0;
  L.rs = L.u + uf / 2;   // (dq is even)
  const int64_t rf = mode == 3 ? (int64_t)L.npass * L.S * n : 0;
  L.total = L.rs + (rf + 1) / 2;
  return L;
}

// ---- the direct-difference derivative kernel (kv_wide_direct_grad.hpp): eight instantiations
template <int KIND>
const void* wide_direct_grad_ptr_kind(int mode) {
  return mode ? reinterpret_cast<const void*>(&kv_wide_direct_grad_kernel<KIND, 1>) : reinterpret_cast<const void*>(&kv_wide_direct_grad_kernel<KIND, 0>);
}
const void* wide_direct_grad_ptr(int kind, int mode) {
  switch (kind) {
    case GPAMD_RBF: return wide_direct_grad_ptr_kind<KIND_RBF>(mode);
    case GPAMD_MATERN12: return wide_direct_grad_ptr_kind<KIND_MATERN12>(mode);
    case GPAMD_MATERN32: return wide_direct_grad_ptr_kind<KIND_MATERN32>(mode);
    case GPAMD_MATERN52: return wide_direct_grad_ptr_kind<KIND_MATERN52>(mode);
  }
  return nullptr;
}

// Split-j plan and workspace: enough (row block of 256, slab) units for one workgroup on each of 256 compute units, slabs of whole 128-row tiles.
// Offsets in doubles: partial sums [npass][nrb S][pstride] | G [S][n][dq] floats (mode 3; the passes add into one)
struct WideDirectGradLayout {
  int nrb, S, jchunk, npass, pstride, dq;
  int64_t g, total;
};
WideDirectGradLayout wide_direct_grad_layout(int n, int m, int d, int t, int mode) {
  WideDirectGradLayout L{};
  L.nrb = (n + KWDG_BM - 1) / KWDG_BM;
  L.dq = kwdg_dq(d);
  const int tiles = kw_tiles(m);
  int S = (256 + L.nrb - 1) / L.nrb;
  S = S < 1 ? 1 : (S > tiles ? tiles : S);
  const int per = (tiles + S - 1) / S;
  L.S = (tiles + per - 1) / per;
  L.jchunk = per * KW_TILE;
  L.npass = (t + KWDG_MAXT - 1) / KWDG_MAXT;
  L.pstride = mode ? 1 + L.dq : 2;
  L.g = ((int64_t)L.npass * L.nrb * L.S * L.pstride + 1) / 2 * 2;
  const int64_t gf = mode == 3 ? (int64_t)L.S * n * L.dq : 0;   // (dq is even)
  L.total = L.g + gf / 2;
  return L;
}

}  // namespace

extern "C" {

int gpamd_wide_split_f32(const float* Xp, int n, int d, int dp, void* image, float* norms, void* stream) {
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, WIDE_DIMS);
  if (!Xp || !image || !norms) return fail(GPAMD_EINVAL, "wide_split: null pointer");
  if (n <= 0 || dp < d || dp % 4) return fail(GPAMD_EINVAL, "wide_split: bad shape (n >= 1, dp >= d, dp % 4 == 0)");
  if (!wide_aligned16(Xp) || !wide_aligned16(image) || !wide_aligned16(norms)) return fail(GPAMD_EINVAL, "wide_split: the rows, the image and the norms must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int tiles = kw_tiles(n), nc = kw_chunks(d);
  hipLaunchKernelGGL(wide_split_kernel, dim3((unsigned)tiles, (unsigned)nc), dim3(256), 0, st, Xp, n, dp, reinterpret_cast<_Float16*>(image), nc);
  hipLaunchKernelGGL(wide_norm_kernel, dim3((unsigned)(tiles * (KW_TILE / 4))), dim3(256), 0, st, Xp, n, dp, norms, tiles * KW_TILE);
  return check_launch("wide_split");
}

int gpamd_kv_wide_plan(int kind, int n, int m, int d, int t, int64_t ldo, int* S_host, int* jchunk_host, int64_t* workspace_floats_host) {
  if (!wide_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_KINDS);
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, WIDE_DIMS);
  if (n <= 0 || m <= 0 || t <= 0 || ldo < n || ldo % 4) return fail(GPAMD_EINVAL, "kv_wide_plan: bad shape (n, m, t >= 1; ldo >= n, ldo % 4 == 0)");
  // the split count and the chunk are the launch plan's own (plan_split behind gpamd_kv_plan), asked for the 128-row geometry of the split-operand
  // kernels (GPAMD_KV_BLOCK128: one row tile per wave, the same j tile); the 32-dimension instantiation it consults runs one wave per SIMD where these
  // run two, so a launch has at least the workgroups the plan counted on
  int S = 0, jc = 0;
  int rc = gpamd_kv_plan(kind, n, m, KV_MAX_DIM, wide_group(t, 0).tg, GPAMD_KV_GRAM | GPAMD_KV_SPLIT | GPAMD_KV_SPLIT_FEW | GPAMD_KV_BLOCK128, ldo, &S, &jc, nullptr);
  if (rc) return rc;
  if (S_host) *S_host = S;
  if (jchunk_host) *jchunk_host = jc;
  if (workspace_floats_host) {
    const WideLayout L = wide_layout(m, t, S, ldo);
    *workspace_floats_host = L.base + L.total;
  }
  return 0;
}

int gpamd_kv_wide_partials_f32(int kind, const void* Z1, const float* N1, int n, const void* Z2, const float* N2, int m, int chunks, const float* Vt,
                               int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (!wide_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_KINDS);
  if (chunks < kw_chunks(KW_MIN_DIM) || chunks > kw_chunks(KW_MAX_DIM)) return fail(GPAMD_EUNSUPPORTED, WIDE_DIMS);
  if (!Z1 || !N1 || !Z2 || !N2 || !Vt || !P) return fail(GPAMD_EINVAL, "kv_wide: null pointer");
  if (n <= 0 || m <= 0 || t <= 0 || S <= 0) return fail(GPAMD_EINVAL, "kv_wide: bad shape (n, m, t, S >= 1)");
  if (ldv % 4 || ldv < m || ldo < n || ldo % 4) return fail(GPAMD_EINVAL, "kv_wide: leading dimensions must be >= extent and multiples of 4");
  if (!wide_aligned16(Z1) || !wide_aligned16(Z2) || !wide_aligned16(N1) || !wide_aligned16(N2) || !wide_aligned16(Vt) || !wide_aligned16(P))
    return fail(GPAMD_EINVAL, "kv_wide: the images, the norms, Vt and the workspace must be 16-byte aligned");
  if (jchunk % KGH_BN || (int64_t)jchunk * S < m) return fail(GPAMD_EINVAL, "kv_wide: jchunk * S must cover m and jchunk % 128 == 0 (use gpamd_kv_wide_plan)");
  hipStream_t st = (hipStream_t)stream;
  const WideLayout L = wide_layout(m, t, S, ldo);
  float* xbase = P + L.base;
  constexpr int ni = KW_NI;
  hipLaunchKernelGGL(wide_clear_kernel, dim3((unsigned)((L.slots + 255) / 256)), dim3(256), 0, st, reinterpret_cast<unsigned*>(xbase + L.colmax), L.slots);
  int64_t prow = 0;   // plane rows used so far
  int mulslot = 0;    // multiplier slots used so far
  for (int g0 = 0; g0 < t;) {
    const WideGroup g = wide_group(t, g0);
    const void* fn = wide_ptr(kind, g.ct, g.ex);
    if (!fn) return fail(GPAMD_EUNSUPPORTED, "kv_wide: no kernel variant for this shape");
    KvWideArgs wa;
    KvhArgs& ka = wa.h;
    KvArgs& a = ka.a;
    a.X1 = nullptr; a.X2 = nullptr;
    a.Vt = Vt + (int64_t)g0 * ldv;
    a.P = P + (int64_t)g0 * ldo;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
    a.n = n; a.m = m; a.t = g.tg;
    a.S = S; a.jchunk = jchunk;
    a.nrb = (n + kgh_bm(ni) - 1) / kgh_bm(ni);
    a.done = done;
    a.kparam = 0.f;
    // pre-pass: per-column scale + the two f16 planes of this group's matrix-pipe columns (the extra column stays f32)
    const int tc = 32 * g.ct;
    unsigned* colmax = reinterpret_cast<unsigned*>(xbase + L.colmax) + mulslot;
    float* colmul = xbase + L.colmul + mulslot;
    _Float16* vh = reinterpret_cast<_Float16*>(xbase + L.planes) + 2 * prow * L.ldh;
    _Float16* vl = vh + (int64_t)tc * L.ldh;
    vsplit_launch(a.Vt, ldv, m, g.tg - g.ex, tc, vh, vl, L.ldh, colmax, colmul, done, st);
    ka.Vh = vh; ka.Vl = vl; ka.ldh = L.ldh; ka.colmul = colmul;
    wa.Z1 = reinterpret_cast<const _Float16*>(Z1); wa.Z2 = reinterpret_cast<const _Float16*>(Z2);
    wa.N1 = N1; wa.N2 = N2; wa.nc = chunks;
    prow += tc;
    mulslot += tc + 1;
    void* kargs[] = {(void*)&wa};
    (void)hipLaunchKernel(fn, dim3((unsigned)a.nrb * (unsigned)S), dim3(256), kargs, 0, st);
    int rc = check_launch("kv_wide_partials");
    if (rc) return rc;
    g0 += g.tg;
  }
  return 0;
}

int gpamd_kv_wide_direct_plan(int kind, int n, int m, int d, int t, int64_t ldo, int* S_host, int* jchunk_host, int64_t* workspace_floats_host) {
  if (!wide_direct_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_KINDS);
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_DIMS);
  if (n <= 0 || m <= 0 || t <= 0 || ldo < n || ldo % 4) return fail(GPAMD_EINVAL, "kv_wide_direct_plan: bad shape (n, m, t >= 1; ldo >= n, ldo % 4 == 0)");
  int S = 0, jc = 0;
  wide_direct_split(n, m, &S, &jc);
  if (S_host) *S_host = S;
  if (jchunk_host) *jchunk_host = jc;
  if (workspace_floats_host) {
    const WideLayout L = wide_layout(m, t, S, ldo);
    *workspace_floats_host = L.base + L.total;
  }
  return 0;
}

int gpamd_kv_wide_direct_partials_f32(int kind, const float* X1p, int n, const float* X2p, int m, int d, int dp, const float* Vt, int64_t ldv, int t, float* P,
                                      int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (!wide_direct_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_KINDS);
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_DIMS);
  if (!X1p || !X2p || !Vt || !P) return fail(GPAMD_EINVAL, "kv_wide_direct: null pointer");
  if (n <= 0 || m <= 0 || t <= 0 || S <= 0 || dp < d || dp % 4) return fail(GPAMD_EINVAL, "kv_wide_direct: bad shape (n, m, t, S >= 1; dp >= d, dp % 4 == 0)");
  if (ldv % 4 || ldv < m || ldo < n || ldo % 4) return fail(GPAMD_EINVAL, "kv_wide_direct: leading dimensions must be >= extent and multiples of 4");
  if (!wide_aligned16(X1p) || !wide_aligned16(X2p) || !wide_aligned16(Vt) || !wide_aligned16(P))
    return fail(GPAMD_EINVAL, "kv_wide_direct: the prepared rows, Vt and the workspace must be 16-byte aligned");
  if (jchunk <= 0 || jchunk % KGH_BN || (int64_t)jchunk * S < m)
    return fail(GPAMD_EINVAL, "kv_wide_direct: jchunk * S must cover m and jchunk % 128 == 0 (use gpamd_kv_wide_direct_plan)");
  hipStream_t st = (hipStream_t)stream;
  const WideLayout L = wide_layout(m, t, S, ldo);
  float* xbase = P + L.base;
  hipLaunchKernelGGL(wide_clear_kernel, dim3((unsigned)((L.slots + 255) / 256)), dim3(256), 0, st, reinterpret_cast<unsigned*>(xbase + L.colmax), L.slots);
  int64_t prow = 0;   // plane rows used so far
  int mulslot = 0;    // multiplier slots used so far
  for (int g0 = 0; g0 < t;) {
    const WideGroup g = wide_group(t, g0);
    const void* fn = wide_direct_ptr(kind, g.ct, g.ex);
    if (!fn) return fail(GPAMD_EUNSUPPORTED, "kv_wide_direct: no kernel variant for this shape");
    KvWideDirectArgs wa;
    KvhArgs& ka = wa.h;
    KvArgs& a = ka.a;
    a.X1 = X1p; a.X2 = X2p;
    a.Vt = Vt + (int64_t)g0 * ldv;
    a.P = P + (int64_t)g0 * ldo;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
    a.n = n; a.m = m; a.t = g.tg;
    a.S = S; a.jchunk = jchunk;
    a.nrb = (n + kgh_bm(KWD_NI) - 1) / kgh_bm(KWD_NI);
    a.done = done;
    a.kparam = 0.f;
    // pre-pass: per-column scale + the two f16 planes of this group's matrix-pipe columns (the extra column stays f32)
    const int tc = 32 * g.ct;
    unsigned* colmax = reinterpret_cast<unsigned*>(xbase + L.colmax) + mulslot;
    float* colmul = xbase + L.colmul + mulslot;
    _Float16* vh = reinterpret_cast<_Float16*>(xbase + L.planes) + 2 * prow * L.ldh;
    _Float16* vl = vh + (int64_t)tc * L.ldh;
    vsplit_launch(a.Vt, ldv, m, g.tg - g.ex, tc, vh, vl, L.ldh, colmax, colmul, done, st);
    ka.Vh = vh; ka.Vl = vl; ka.ldh = L.ldh; ka.colmul = colmul;
    wa.dp = dp; wa.nc = kw_chunks(d);
    prow += tc;
    mulslot += tc + 1;
    void* kargs[] = {(void*)&wa};
    (void)hipLaunchKernel(fn, dim3((unsigned)a.nrb * (unsigned)S), dim3(256), kargs, 0, st);
    int rc = check_launch("kv_wide_direct_partials");
    if (rc) return rc;
    g0 += g.tg;
  }
  return 0;
}

int64_t gpamd_kv_wide_direct_grad_workspace_doubles(int n, int m, int d, int t, int mode) {
  if (n <= 0 || m <= 0 || t <= 0 || d < KW_MIN_DIM || d > KW_MAX_DIM || mode < 0 || mode > 3 || mode == 2) return 0;
  return wide_direct_grad_layout(n, m, d, t, mode).total;
}

int gpamd_kv_wide_direct_grad_f32(int kind, const float* X1p, int n, const float* X2p, int m, int d, int dp, const float* Lt, int64_t ldl, const float* Rt,
                                  int64_t ldr, int t, int mode, float* out, float* Gz1, int64_t ldg, double* ws, int64_t ws_doubles, void* stream) {
  if (!wide_direct_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_KINDS);
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, WIDE_DIRECT_DIMS);
  if (mode < 0 || mode > 3 || mode == 2)
    return fail(GPAMD_EINVAL, "kv_wide_direct_grad: mode is 0 (one lengthscale), 1 (per dimension) or 3 (per dimension + Gz1)");
  if (!X1p || !X2p || !Lt || !Rt || !out || !ws) return fail(GPAMD_EINVAL, "kv_wide_direct_grad: null pointer");
  if (mode == 3 && (!Gz1 || ldg < d)) return fail(GPAMD_EINVAL, "kv_wide_direct_grad: Gz1 [n][ldg >= d] missing");
  if (n <= 0 || m <= 0 || t <= 0 || dp < d || dp % 4 || ldl < n || ldr < m)
    return fail(GPAMD_EINVAL, "kv_wide_direct_grad: bad shape (n, m, t >= 1; dp >= d, dp % 4 == 0; ldl >= n; ldr >= m)");
  if (!wide_aligned16(X1p) || !wide_aligned16(X2p) || !wide_aligned16(ws))
    return fail(GPAMD_EINVAL, "kv_wide_direct_grad: the prepared rows and the workspace must be 16-byte aligned");
  const WideDirectGradLayout L = wide_direct_grad_layout(n, m, d, t, mode);
  if (ws_doubles < L.total) return fail(GPAMD_EWORKSPACE, "kv_wide_direct_grad: workspace too small (gpamd_kv_wide_direct_grad_workspace_doubles)");
  hipStream_t st = (hipStream_t)stream;
  const void* fn = wide_direct_grad_ptr(kind, mode ? 1 : 0);
  float* G = mode == 3 ? reinterpret_cast<float*>(ws + L.g) : nullptr;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kwdg_lds(KWDG_MAXT, kwdg_dq(KW_MAX_DIM), 1));
  for (int p = 0; p < L.npass; ++p) {
    KvWideDirectGradArgs a;
    a.X1 = X1p; a.X2 = X2p;
    a.Lt = Lt + (int64_t)p * KWDG_MAXT * ldl; a.Rt = Rt + (int64_t)p * KWDG_MAXT * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.dp = dp; a.nc = kw_chunks(d);
    a.tp = t - p * KWDG_MAXT < KWDG_MAXT ? t - p * KWDG_MAXT : KWDG_MAXT;
    a.tpad = (a.tp + 1) / 2 * 2;
    a.S = L.S; a.jchunk = L.jchunk; a.nrb = L.nrb;
    a.part = ws + (int64_t)p * L.nrb * L.S * L.pstride;
    a.pstride = L.pstride;
    a.G = G; a.dq = L.dq; a.add = p > 0;
    void* kargs[] = {(void*)&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)(L.nrb * L.S)), dim3(256), kargs, kwdg_lds(a.tpad, L.dq, mode ? 1 : 0), st);
    int rc = check_launch("kv_wide_direct_grad");
    if (rc) return rc;
  }
  const int nout = 2 + dp;
  hipLaunchKernelGGL(wide_direct_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, ws, L.npass * L.nrb * L.S, L.pstride,
                     mode ? 1 : 0, d, out, nout);
  if (mode == 3)
    hipLaunchKernelGGL(wide_direct_gz_reduce_kernel, dim3((unsigned)(((int64_t)n * d + 255) / 256)), dim3(256), 0, st, G, L.S, n, d, L.dq, Gz1, ldg);
  return check_launch("kv_wide_direct_grad reduce");
}

int64_t gpamd_kv_wide_grad_workspace_doubles(int n, int m, int d, int t, int mode) {
  if (n <= 0 || m <= 0 || t <= 0 || d < KW_MIN_DIM || d > KW_MAX_DIM) return 0;
  return wide_grad_layout(n, m, d, t, mode).total;
}

int gpamd_wide_split_t_f32(const float* Xp, int n, int d, int dp, void* timage, void* stream) {
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EINVAL, WIDE_DIMS);
  if (!Xp || !timage) return fail(GPAMD_EINVAL, "wide_split_t: null pointer");
  if (n <= 0 || dp < d) return fail(GPAMD_EINVAL, "wide_split_t: bad shape (n >= 1, dp >= d)");
  if (!wide_aligned16(timage)) return fail(GPAMD_EINVAL, "wide_split_t: the image must be 16-byte aligned");
  hipLaunchKernelGGL(wide_split_t_kernel, dim3((unsigned)kw_tiles(n), (unsigned)(2 * kwg_dblocks(d))), dim3(256), 0, (hipStream_t)stream, Xp, n, d, dp,
                     reinterpret_cast<_Float16*>(timage));
  return check_launch("wide_split_t");
}

int gpamd_kv_wide_grad_f32(int kind, const void* Z1, const float* N1, const float* X1p, int n, const void* Z2, const float* N2, const void* T2, int m, int d,
                           int dp, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t, int mode, const float* wscale, float* out, float* Gz1,
                           int64_t ldg, double* ws, int64_t ws_doubles, void* stream) {
  if (!wide_kind_ok(kind)) return fail(GPAMD_EUNSUPPORTED, WIDE_KINDS);
  if (d < KW_MIN_DIM || d > KW_MAX_DIM) return fail(GPAMD_EINVAL, WIDE_DIMS);
  if (mode < 0 || mode > 3 || mode == 2) return fail(GPAMD_EINVAL, "kv_wide_grad: mode is 0 (one lengthscale), 1 (per dimension) or 3 (per dimension + Gz1)");
  if (!Z1 || !N1 || !Z2 || !N2 || !Lt || !Rt || !wscale || !out || !ws) return fail(GPAMD_EINVAL, "kv_wide_grad: null pointer");
  if (mode && (!T2 || !X1p)) return fail(GPAMD_EINVAL, "kv_wide_grad: the per-dimension modes need the transposed image of x2 and the prepared rows of x1");
  if (mode == 3 && (!Gz1 || ldg < d)) return fail(GPAMD_EINVAL, "kv_wide_grad: Gz1 [n][ldg >= d] missing");
  if (n <= 0 || m <= 0 || t <= 0 || dp < d || ldl < n || ldr < m) return fail(GPAMD_EINVAL, "kv_wide_grad: bad shape (n, m, t >= 1; dp >= d; ldl >= n; ldr >= m)");
  if (!wide_aligned16(Z1) || !wide_aligned16(Z2) || !wide_aligned16(N1) || !wide_aligned16(N2) || !wide_aligned16(ws) || (T2 && !wide_aligned16(T2)))
    return fail(GPAMD_EINVAL, "kv_wide_grad: the images, the norms and the workspace must be 16-byte aligned");
  const WideGradLayout L = wide_grad_layout(n, m, d, t, mode);
  if (ws_doubles < L.total) return fail(GPAMD_EWORKSPACE, "kv_wide_grad: workspace too small (gpamd_kv_wide_grad_workspace_doubles)");
  hipStream_t st = (hipStream_t)stream;
  const void* fn = wide_grad_ptr(kind, mode ? 1 : 0);
  float* U = mode == 3 ? reinterpret_cast<float*>(ws + L.u) : nullptr;
  float* RS = mode == 3 ? reinterpret_cast<float*>(ws + L.rs) : nullptr;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kwg_lds(KWG_MAXT));
  for (int p = 0; p < L.npass; ++p) {
    KvWideGradArgs a;
    a.Z1 = reinterpret_cast<const _Float16*>(Z1); a.Z2 = reinterpret_cast<const _Float16*>(Z2); a.T2 = reinterpret_cast<const _Float16*>(T2);
    a.N1 = N1; a.N2 = N2; a.X1 = X1p;
    a.Lt = Lt + (int64_t)p * KWG_MAXT * ldl; a.Rt = Rt + (int64_t)p * KWG_MAXT * ldr;
    a.ldl = ldl; a.ldr = ldr;
    a.n = n; a.m = m; a.dp = dp; a.nc = kw_chunks(d);
    a.tp = t - p * KWG_MAXT < KWG_MAXT ? t - p * KWG_MAXT : KWG_MAXT;
    a.tpad = (a.tp + 1) / 2 * 2;
    a.S = L.S; a.jchunk = L.jchunk; a.nrb = L.nrb;
    a.wscale = wscale;
    a.part = ws + (int64_t)p * L.nrb * L.S * L.pstride;
    a.pstride = L.pstride;
    a.dq = L.dq;
    a.U = U ? U + (int64_t)p * L.S * n * L.dq : nullptr;
    a.RS = RS ? RS + (int64_t)p * L.S * n : nullptr;
    void* kargs[] = {(void*)&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)(L.nrb * L.S), (unsigned)(mode ? L.ndb : 1)), dim3(256), kargs, kwg_lds(a.tpad), st);
    int rc = check_launch("kv_wide_grad");
    if (rc) return rc;
  }
  const int nout = 2 + dp;
  hipLaunchKernelGGL(wide_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, ws, L.npass * L.nrb * L.S, L.pstride, mode ? 1 : 0, d,
                     wscale, out, nout);
  if (mode == 3)
    hipLaunchKernelGGL(wide_gz_reduce_kernel, dim3((unsigned)(((int64_t)n * d + 255) / 256)), dim3(256), 0, st, U, RS, L.npass * L.S, n, d, L.dq, X1p, dp,
                       wscale, Gz1, ldg);
  return check_launch("kv_wide_grad reduce");
}

}  // extern "C"
