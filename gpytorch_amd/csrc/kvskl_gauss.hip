// The symmetrized-KL kernels over Gaussian inputs (kv_directskl.hpp): prepared width 4, 12 and 20, NI = 1, 2 row tiles per wave (width 20: 1), without /
// with the extra VALU column.
#include "host.hpp"
#include "kv_directskl.hpp"

namespace gpamd {

namespace {
template <int W>
const void* directskl_ptr(int ni, int ex) {
#define KSK_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directskl_kernel<W, N, E>);
  KSK_CASE(1, 0) KSK_CASE(1, 1)
  if constexpr (ksk_ni(false, W) == 2) { KSK_CASE(2, 0) KSK_CASE(2, 1) }   // (width 20 has one row tile per wave: ksk_ni)
#undef KSK_CASE
  return nullptr;
}
}  // namespace

// width: the prepared width (4, 12, 20); ni: 32-row tiles per wave; ex: extra VALU column
const void* kvskl_kernel_ptr_gauss(int width, int ni, int ex) {
  if (width == 4) return directskl_ptr<4>(ni, ex);
  if (width == 12) return directskl_ptr<12>(ni, ex);
  if (width == 20) return directskl_ptr<20>(ni, ex);
  return nullptr;
}

}  // namespace gpamd
