// The Gibbs kernels (kv_directgibbs.hpp): prepared width 4 and 8, NI = 1, 2 row tiles per wave, without / with the extra VALU column.
#include "host.hpp"
#include "kv_directgibbs.hpp"

namespace gpamd {

namespace {
template <int W>
const void* directgibbs_ptr(int ni, int ex) {
#define KGB_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directgibbs_kernel<W, N, E>);
  KGB_CASE(1, 0) KGB_CASE(1, 1) KGB_CASE(2, 0) KGB_CASE(2, 1)
#undef KGB_CASE
  return nullptr;
}
}  // namespace

// width: the prepared width (4, 8); ni: 32-row tiles per wave; ex: extra VALU column
const void* kvg_kernel_ptr_gibbs(int width, int ni, int ex) {
  if (width == 4) return directgibbs_ptr<4>(ni, ex);
  if (width == 8) return directgibbs_ptr<8>(ni, ex);
  return nullptr;
}

}  // namespace gpamd
