// The linear model of coregionalisation (kv_lcm.hpp): the fused multi-member product kernels for D = 2, 3, 4 (d = 1 runs on D = 2: its second coordinate and
// weight are zero), Q = 1..4 members, NI = 1, 2 row tiles per wave; the mixing pre-pass for T = 2..8 tasks; and the entry points gpamd_kv_lcm_*.
#include "host.hpp"
#include "kv_lcm.hpp"

using namespace gpamd;

namespace {

template <int D, int Q>
const void* lcm_ptr_ni(int ni) {
  if (ni == 1) return reinterpret_cast<const void*>(&kv_lcm_kernel<D, Q, 1>);
  if (ni == 2) return reinterpret_cast<const void*>(&kv_lcm_kernel<D, Q, 2>);
  return nullptr;
}
template <int D>
const void* lcm_ptr_q(int q, int ni) {
  switch (q) {
    case 1: return lcm_ptr_ni<D, 1>(ni);
    case 2: return lcm_ptr_ni<D, 2>(ni);
    case 3: return lcm_ptr_ni<D, 3>(ni);
    case 4: return lcm_ptr_ni<D, 4>(ni);
  }
  return nullptr;
}
const void* lcm_ptr(int d, int q, int ni) {
  switch (d) {
    case 1:
    case 2: return lcm_ptr_q<2>(q, ni);
    case 3: return lcm_ptr_q<3>(q, ni);
    case 4: return lcm_ptr_q<4>(q, ni);
  }
  return nullptr;
}

bool lcm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
const char* lcm_shape_error(int d, int q, int tasks) {
  if (d < 1 || d > KLC_MAX_DIM) return "kv_lcm: d outside the native envelope 1..4";
  if (q < 1 || q > KLC_MAX_MEMBERS) return "kv_lcm: Q outside the native envelope 1..4";
  if (tasks < KLC_MIN_TASKS || tasks > KLC_MAX_TASKS) return "kv_lcm: T outside the native envelope 2..8";
  return nullptr;
}

// Behind the S interleaved slabs: the column maxima and multipliers of every launch group (32 each), then each group's two f16 planes of Q x 32 rows.
// Offsets in floats, multiples of 4
struct LcmLayout {
  int64_t base, colmax, colmul, planes, total, ldh;
  int groups, per_group;
};
LcmLayout lcm_layout(int m, int q, int tasks, int probes, int S, int64_t ldo) {
  LcmLayout L{};
  L.per_group = klc_probes(tasks);
  L.groups = (probes + L.per_group - 1) / L.per_group;
  L.base = ((int64_t)S * probes * ldo + 3) / 4 * 4;
  L.ldh = ((int64_t)m + KGH_BN - 1) / KGH_BN * KGH_BN;
  L.colmax = 0;
  L.colmul = (int64_t)KLC_COLS * L.groups;
  L.planes = 2 * L.colmul;
  L.total = L.planes + (int64_t)L.groups * q * KLC_COLS * L.ldh;   // two f16 planes of Q x 32 rows = Q x 32 x ldh floats
  return L;
}

template <int T>
void lcm_prepass(const float* Vi, int64_t ldv, int m, int probes, int q, const float* par, _Float16* vh, _Float16* vl, int64_t ldh, unsigned* colmax,
                 float* colmul, const int* done, hipStream_t st) {
  unsigned nbm = (unsigned)((m + 4095) / 4096);
  if (nbm > 64) nbm = 64;
  hipLaunchKernelGGL(lcm_colmax_kernel<T>, dim3(nbm, probes), dim3(256), 0, st, Vi, ldv, m, q, par, colmax, done);
  hipLaunchKernelGGL(lcm_mix_split_kernel<T>, dim3((unsigned)((ldh / 8 + 255) / 256), probes), dim3(256), 0, st, Vi, ldv, m, probes, q, par, vh, vl, ldh,
                     (const unsigned*)colmax, colmul, done);
}

}  // namespace

extern "C" {

int gpamd_kv_lcm_plan(int n, int m, int d, int q, int tasks, int probes, int64_t ldo, int* S_host, int* jchunk_host, int64_t* workspace_floats_host) {
  if (const char* bad = lcm_shape_error(d, q, tasks)) return fail(GPAMD_EUNSUPPORTED, bad);
  if (n <= 0 || m <= 0 || probes <= 0 || (int64_t)n * tasks > 0x7fffffff || (int64_t)m * tasks > 0x7fffffff || ldo < (int64_t)n * tasks || ldo % 4)
    return fail(GPAMD_EINVAL, "kv_lcm_plan: bad shape (n, m, probes >= 1; n T and m T below 2^31; ldo >= n T, ldo % 4 == 0)");
  // the split count and the chunk are the launch plan's own (plan_split behind gpamd_kv_plan): the kernels share tile, row-tile rule and launch
  // bounds with the Gibbs family's direct-difference kernels at the prepared width 4
  int S = 0, jc = 0;
  const int cols = probes < klc_probes(tasks) ? probes * tasks : klc_probes(tasks) * tasks;
  int rc = gpamd_kv_plan(GPAMD_GIBBS, n, m, 4, cols, GPAMD_KV_SPLIT, (n + 3) / 4 * 4, &S, &jc, nullptr);
  if (rc) return rc;
  if (S_host) *S_host = S;
  if (jchunk_host) *jchunk_host = jc;
  if (workspace_floats_host) {
    const LcmLayout L = lcm_layout(m, q, tasks, probes, S, ldo);
    *workspace_floats_host = L.base + L.total;
  }
  return 0;
}

int gpamd_kv_lcm_partials_f32(const float* block, int q, int d, int tasks, const float* X1c, int n, const float* X2c, int m, const float* Vi, int64_t ldv,
                              int probes, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (const char* bad = lcm_shape_error(d, q, tasks)) return fail(GPAMD_EUNSUPPORTED, bad);
  if (!block || !X1c || !X2c || !Vi || !P) return fail(GPAMD_EINVAL, "kv_lcm: null pointer");
  if (n <= 0 || m <= 0 || probes <= 0 || S <= 0 || (int64_t)n * tasks > 0x7fffffff || (int64_t)m * tasks > 0x7fffffff)
    return fail(GPAMD_EINVAL, "kv_lcm: bad shape (n, m, probes, S >= 1; n T and m T below 2^31)");
  if (ldv < (int64_t)m * tasks || ldo < (int64_t)n * tasks || ldo % 4)
    return fail(GPAMD_EINVAL, "kv_lcm: leading dimensions must be >= extent x T and ldo % 4 == 0");
  if (!lcm_aligned16(X1c) || !lcm_aligned16(X2c) || !lcm_aligned16(P)) return fail(GPAMD_EINVAL, "kv_lcm: the points and the workspace must be 16-byte aligned");
  if (jchunk % KGH_BN || (int64_t)jchunk * S < m) return fail(GPAMD_EINVAL, "kv_lcm: jchunk * S must cover m and jchunk % 128 == 0 (use gpamd_kv_lcm_plan)");
  hipStream_t st = (hipStream_t)stream;
  const LcmLayout L = lcm_layout(m, q, tasks, probes, S, ldo);
  float* xbase = P + L.base;
  const int ni = klc_ni(n < KGH_SMALL_N);
  const void* fn = lcm_ptr(d, q, ni);
  if (!fn) return fail(GPAMD_EUNSUPPORTED, "kv_lcm: no kernel variant for this shape");
  unsigned* colmax_all = reinterpret_cast<unsigned*>(xbase + L.colmax);
  const int nmax = KLC_COLS * L.groups;
  hipLaunchKernelGGL(lcm_clear_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, st, colmax_all, nmax);   // (a kernel, not a memset node)
  for (int g = 0; g < L.groups; ++g) {
    const int p0 = g * L.per_group;
    const int pg = probes - p0 < L.per_group ? probes - p0 : L.per_group;
    unsigned* colmax = colmax_all + KLC_COLS * g;
    float* colmul = xbase + L.colmul + KLC_COLS * g;
    _Float16* vh = reinterpret_cast<_Float16*>(xbase + L.planes) + 2 * (int64_t)g * q * KLC_COLS * L.ldh;
    _Float16* vl = vh + (int64_t)q * KLC_COLS * L.ldh;
    const float* Vg = Vi + (int64_t)p0 * ldv;
    switch (tasks) {
#define KLC_CASE(T) case T: lcm_prepass<T>(Vg, ldv, m, pg, q, block, vh, vl, L.ldh, colmax, colmul, done, st); break;
      KLC_CASE(2) KLC_CASE(3) KLC_CASE(4) KLC_CASE(5) KLC_CASE(6) KLC_CASE(7) KLC_CASE(8)
#undef KLC_CASE
    }
    KvLcmArgs ka;
    KvArgs& a = ka.a;
    a.X1 = X1c; a.X2 = X2c; a.Vt = nullptr;
    a.P = P + (int64_t)p0 * ldo;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)probes * ldo;
    a.n = n; a.m = m; a.t = pg * tasks;
    a.S = S; a.jchunk = jchunk;
    a.nrb = (n + kdh_bm(ni) - 1) / kdh_bm(ni);
    a.done = done;
    a.kparam = 0.f;
    ka.Vh = vh; ka.Vl = vl; ka.ldh = L.ldh; ka.colmul = colmul; ka.par = block; ka.tasks = tasks;
    void* kargs[] = {(void*)&ka};
    (void)hipLaunchKernel(fn, dim3((unsigned)a.nrb * (unsigned)S), dim3(256), kargs, 0, st);
    int rc = check_launch("kv_lcm_partials");
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
