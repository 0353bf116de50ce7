// libgpamd_tune.so: the staging arms of kv_gram_kernel (kv_gram.hpp, template parameter STG) side by side -- the product library instantiates only
// KV_GRAM_STAGE.  scripts/kv_gram_stage_ab.py times them against each other on one box; tests/test_gpu_kv_staging.py compares their partial slabs bitwise
// with arm 0 (the staging up to round 6).  Arm 3 of the plan (64-j tiles, two LDS buffers filled by LDS-DMA) is not built.
// The same unit, compiled a second time with GPAMD_KV_STAMP (tune_stage_stamp.o), gives the diagnostic builds with s_memtime stamps around the staging
// span of every tile: gpamd_tune_stage_stamp_launch.
#ifdef GPAMD_KV_STAMP
#define gpamd gpamd_stamp
#else
#define gpamd gpamd_stg
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kv_gram.hpp"

using namespace gpamd;

template <int STG>
static int stage_launch(int variant, KvArgs& a, int S, hipStream_t st) {
  a.nrb = (a.n + 255) / 256;   // NI = 2
  const dim3 grid((unsigned)a.nrb * S), block(256);
  if (variant == 0) hipLaunchKernelGGL((kv_gram_kernel<KIND_RBF, 3, 2, 2, 1, 0, STG>), grid, block, 0, st, a);
  else if (variant == 1) hipLaunchKernelGGL((kv_gram_kernel<KIND_MATERN52, 10, 2, 2, 1, 0, STG>), grid, block, 0, st, a);
  else return -2;
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

static KvArgs stage_args(const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk) {
  KvArgs a;
  a.X1 = X1p; a.X2 = X2p; a.Vt = Vt; a.P = P;
  a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
  a.n = n; a.m = m; a.t = t; a.S = S; a.jchunk = jchunk; a.done = nullptr; a.kparam = 0.f; a.Xc = nullptr;
  return a;
}

#ifndef GPAMD_KV_STAMP
// bit s set: staging arm s is built
extern "C" int gpamd_tune_stage_arms() { return 0b111; }

// variant: 0 = RBF, d = 3; 1 = Matern-5/2, d = 10 (both CT = 2, NI = 2, EX = 1: t must be 65); stage: the STG of kv_gram.hpp
extern "C" int gpamd_tune_stage_launch(int variant, int stage, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P,
                                       int64_t ldo, int S, int jchunk, void* stream) {
  if (t != 65 || jchunk % KV_BN) return -1;
  KvArgs a = stage_args(X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk);
  hipStream_t st = (hipStream_t)stream;
  switch (stage) {
    case 0: return stage_launch<0>(variant, a, S, st);
    case 1: return stage_launch<1>(variant, a, S, st);
    case 2: return stage_launch<2>(variant, a, S, st);
  }
  return -3;
}
#else
// stamped diagnostic builds of arms 0 and 1 (RBF, d = 3 only); after the launch has completed, stamps_out receives kv_stamp_words() 64-bit words:
// per wave of the first KV_STAMP_WG workgroups [cycles barrier 1 -> barrier 2, cycles barrier 2 -> next barrier 1, tiles, 0]
extern "C" int gpamd_tune_stage_stamp_words() { return KV_STAMP_WG * 4 * 4; }
extern "C" int gpamd_tune_stage_stamp_launch(int stage, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P,
                                             int64_t ldo, int S, int jchunk, void* stream, unsigned long long* stamps_out) {
  if (t != 65 || jchunk % KV_BN) return -1;
  KvArgs a = stage_args(X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk);
  hipStream_t st = (hipStream_t)stream;
  int rc = stage == 0 ? stage_launch<0>(0, a, S, st) : stage == 1 ? stage_launch<1>(0, a, S, st) : -3;
  if (rc) return rc;
  hipError_t e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipMemcpyFromSymbol(stamps_out, HIP_SYMBOL(kv_stamp_buf), sizeof(unsigned long long) * KV_STAMP_WG * 4 * 4);
  return e == hipSuccess ? 0 : (int)e;
}
#endif
