// Fused float64 K*V for prepared strides 20 .. 512 (kv_f64_wide.hpp): the kernel's instantiations, its launch plan and its launch.  No entry point of
// its own: gpamd_kv_plan_f64 / gpamd_kv_partials_f64 (extra_f64.hip) call in here for strides beyond 16.
#include "host.hpp"
#include "kv_f64_wide.hpp"

using namespace gpamd;

namespace {

// the families with a bounded dk/ds at s = 0 (kv_f64_wide.hpp, "Accuracy")
constexpr unsigned KINDS_W64 = kind_bit(GPAMD_RBF) | kind_bit(GPAMD_RQ) | kind_bit(GPAMD_MATERN32) | kind_bit(GPAMD_MATERN52);

template <int KIND>
const void* kw64_ptr_kind(int ct, int tv) {
  switch (ct) {
    case 0: return tv == 1 ? reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 0, 1>) : reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 0, 4>);
    case 1: return reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 1, 0>);
    case 2: return reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 2, 0>);
    case 3: return reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 3, 0>);
    case 4: return reinterpret_cast<const void*>(&kv_f64w_kernel<KIND, 4, 0>);
  }
  return nullptr;
}
const void* kw64_ptr(int kind, int ct, int tv) {
  const void* fn = nullptr;
  with_kind<KINDS_W64>(kind, [&](auto K) { fn = kw64_ptr_kind<K()>(ct, tv); });
  return fn;
}

}  // namespace

namespace gpamd {

bool kv64w_stride_ok(int dp) { return dp % 4 == 0 && dp >= KW64_MIN_DP && dp <= KW64_MAX_DP; }
bool kv64w_kind_ok(int kind) { return kind_accepted(kind, KINDS_W64); }

// The rule of gpamd_kv_plan_f64 on 128-row blocks: about three rounds of the two resident workgroups per CU, chunks of whole 64-row j tiles, at least
// four tiles per chunk (every chunk stages its i block once per tile and writes a slab)
void kv64w_plan(int n, int m, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_doubles) {
  const int nrb = (n + KW64_BM - 1) / KW64_BM;
  int s = (3 * 2 * num_cus() + nrb - 1) / nrb;
  const int smax = m / (4 * KW64_BN) > 0 ? m / (4 * KW64_BN) : 1;
  if (s > smax) s = smax;
  const int jc = ((m + s - 1) / s + KW64_BN - 1) / KW64_BN * KW64_BN;
  *jchunk = jc;
  *S = (m + jc - 1) / jc;
  *workspace_doubles = (int64_t)(*S) * t * ldo;
}

int kv64w_launch(int kind, double kparam, const double* X1p, int n, const double* X2p, int m, int dp, const double* Vt, int64_t ldv, int t, double* P,
                 int64_t ldo, int S, int jchunk, const int* done, hipStream_t stream) {
  if (((reinterpret_cast<uintptr_t>(X1p) | reinterpret_cast<uintptr_t>(X2p)) & 15) != 0)
    return fail(GPAMD_EINVAL, "kv_partials_f64: prepared clouds of more than 16 columns must be 16-byte aligned");
  // groups of <= 64 columns; a group of <= 4 (a remainder, or the whole product) contracts on the VALU
  for (int g0 = 0; g0 < t;) {
    const int tg = t - g0 < KW64_MAX_GROUP ? t - g0 : KW64_MAX_GROUP;
    KvArgsW64 a;
    a.X1 = X1p; a.X2 = X2p;
    a.Vt = Vt + (int64_t)g0 * ldv;
    a.P = P + (int64_t)g0 * ldo;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
    a.n = n; a.m = m; a.t = tg; a.dp = dp;
    a.S = S; a.jchunk = jchunk;
    a.nrb = (n + KW64_BM - 1) / KW64_BM;
    a.done = done;
    a.kparam = kparam;
    const void* fn = tg <= 4 ? kw64_ptr(kind, 0, tg == 1 ? 1 : 4) : kw64_ptr(kind, (tg + 15) / 16, 0);
    if (!fn) return fail(GPAMD_EUNSUPPORTED, "kv_f64: no kernel variant");
    void* kargs[] = {(void*)&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)a.nrb * (unsigned)S), dim3(256), kargs, 0, stream);
    g0 += tg;
  }
  return check_launch("kv_partials_f64");
}

}  // namespace gpamd
