// Included by kvsm_<name>.hip with GPAMD_SM_D (input dimensions), GPAMD_SM_Q0 (first of FOUR consecutive mixture counts) and GPAMD_NAME defined: the
// spectral-mixture kernels (kv_directsm.hpp) of those (Q, d), NI = 1, 2 row tiles per wave (ksm_ni), without / with the extra VALU column.
#include "host.hpp"
#include "kv_directsm.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int Q>
const void* directsm_ptr(int ni, int ex) {
#define KSM_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directsm_kernel<Q, GPAMD_SM_D, N, E>);
  KSM_CASE(1, 0) KSM_CASE(1, 1)
  if constexpr (ksm_ni(false, ksm_width(Q, GPAMD_SM_D)) == 2) { KSM_CASE(2, 0) KSM_CASE(2, 1) }
#undef KSM_CASE
  return nullptr;
}
}  // namespace

// q: mixtures (GPAMD_SM_Q0 .. GPAMD_SM_Q0 + 3); ni: 32-row tiles per wave; ex: extra VALU column
const void* GPAMD_CAT(kvsm_kernel_ptr_, GPAMD_NAME)(int q, int ni, int ex) {
  switch (q - GPAMD_SM_Q0) {
    case 0: return directsm_ptr<GPAMD_SM_Q0>(ni, ex);
    case 1: return directsm_ptr<GPAMD_SM_Q0 + 1>(ni, ex);
    case 2: return directsm_ptr<GPAMD_SM_Q0 + 2>(ni, ex);
    case 3: return directsm_ptr<GPAMD_SM_Q0 + 3>(ni, ex);
  }
  return nullptr;
}

}  // namespace gpamd
