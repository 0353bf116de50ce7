// Included by kv_<family>.hip with GPAMD_KIND / GPAMD_NAME defined: instantiates the fused K*V kernels of
// one covariance family and exposes ONE lookup, kernel pointer by (mode, valid dims, column variant).
#include "host.hpp"
#include "kv_gram.hpp"
#include "kv_valu.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {

template <int D>
const void* mfma_ptr(int ct, int ex) {
#define L(CT, EX) \
  if (ct == CT && ex == EX) return reinterpret_cast<const void*>(&kv_mfma_kernel<GPAMD_KIND, D, CT, kv_ni_for_ct(CT, D), EX>);
  L(1, 0) L(1, 1) L(2, 0) L(2, 1) L(3, 0) L(3, 1) L(4, 0) L(4, 1)
#undef L
  return nullptr;
}

template <int D>
const void* gram_ptr(int ct, int ex) {
#ifndef GPAMD_NO_GRAM
#define L(CT, EX) \
  if (ct == CT && ex == EX) return reinterpret_cast<const void*>(&kv_gram_kernel<GPAMD_KIND, D, CT, kv_ni_for_ct(CT, D), EX>);
  L(1, 0) L(1, 1) L(2, 0) L(2, 1) L(3, 0) L(3, 1) L(4, 0) L(4, 1)
#undef L
#endif
  return nullptr;
}

template <int D>
const void* valu_ptr(int tpad) {
#define L(T) \
  if (tpad == T) return reinterpret_cast<const void*>(&kv_valu_kernel<GPAMD_KIND, D, T>);
  L(1) L(2) L(4) L(8)
  // 9 .. 16 columns WITHOUT the Gram form (direct differences: Matern-1/2, clouds outside the expansion's accuracy policy, the wide rows of a
  // block-centred product): the packed-f32 VALU contraction beats a 32-column matrix-pipe tile that is two thirds padding -- measured on the road3d-shaped
  // workload (n = 217 437, Matern-5/2, 11 columns: kv_mfma<CT = 1> 33 ms per product, kv_valu<T = 16> 27 ms; profiles/r05_s1 / r05_s4_workload_road3d_kernel_stats.csv).
  // Up to 4 dimensions: with more, generation dominates and the matrix-pipe tile wins (d = 10: 0.83 against 1.16 ms on the protein shape's wide rows)
  if constexpr (D <= 4) { L(16) }
#undef L
  return nullptr;
}

template <int D>
const void* any_ptr(int mode, int v, int ex) {
  switch (mode) {
    case KV_MODE_MFMA: return mfma_ptr<D>(v, ex);
    case KV_MODE_GRAM: return gram_ptr<D>(v, ex);
    case KV_MODE_VALU: return valu_ptr<D>(v);
  }
  return nullptr;
}

}  // namespace

// mode: KV_MODE_*; d: valid dims (one of 1,2,3,4,5,6,8,10,12,16,20,24,32: kv_kernel_dims); v: CT (mfma / gram) or padded t (valu); KV_MODE_GRAMV lives in kvs_family.inc
const void* GPAMD_CAT(kv_kernel_ptr_, GPAMD_NAME)(int mode, int d, int v, int ex) {
  const void* fn = nullptr;
  with_dim(d, [&](auto D) { fn = any_ptr<D()>(mode, v, ex); });
  return fn;
}

}  // namespace gpamd
