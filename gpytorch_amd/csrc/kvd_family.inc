// Included by kvd_<family>.hip with GPAMD_KIND / GPAMD_NAME defined: the direct-difference + split-contraction kernels of one covariance family
// (kv_directh.hpp: squared distances on the packed-f32 pipe, contraction on the f16 matrix pipe).  One or two 32-column tiles (+ the extra VALU column); NI = 2 row tiles per wave,
// 1 for few output rows and for two column tiles beyond four dimensions.
#include "host.hpp"
#include "kv_directh.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D>
const void* directh_ptr(int ni, int ct, int ex) {
#define KDH_CASE(N, C, E) if (ni == N && ct == C && ex == E) return reinterpret_cast<const void*>(&kv_directh_kernel<GPAMD_KIND, D, N, C, E>);
  KDH_CASE(1, 1, 0) KDH_CASE(1, 1, 1) KDH_CASE(2, 1, 0) KDH_CASE(2, 1, 1) KDH_CASE(1, 2, 0) KDH_CASE(1, 2, 1)
  if constexpr (kdh_ni(false, 2, D) == 2) { KDH_CASE(2, 2, 0) KDH_CASE(2, 2, 1) }
#undef KDH_CASE
  return nullptr;
}
}  // namespace

// d: valid dims (one of 1,2,3,4,5,6,8,10); ni: 32-row tiles per wave; ct: 32-column tiles (1, 2); ex: extra VALU column
const void* GPAMD_CAT(kvd_kernel_ptr_, GPAMD_NAME)(int d, int ni, int ct, int ex) {
  const void* fn = nullptr;
  with_dim<KDH_MAX_DIM>(d, [&](auto D) { fn = directh_ptr<D()>(ni, ct, ex); });
  return fn;
}

}  // namespace gpamd
