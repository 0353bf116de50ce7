// The Hamming kernels (kv_directham.hpp): prepared width 4, 8, 16 and 32 dwords, NI = 1, 2 row tiles per wave, without / with the extra VALU column.
#include "host.hpp"
#include "kv_directham.hpp"

namespace gpamd {

namespace {
template <int W>
const void* directham_ptr(int ni, int ex) {
#define KHM_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directham_kernel<W, N, E>);
  KHM_CASE(1, 0) KHM_CASE(1, 1) KHM_CASE(2, 0) KHM_CASE(2, 1)
#undef KHM_CASE
  return nullptr;
}
}  // namespace

// width: the prepared width in dwords (4, 8, 16, 32); ni: 32-row tiles per wave; ex: extra VALU column
const void* kvham_kernel_ptr_packed(int width, int ni, int ex) {
  switch (width) {
    case 4: return directham_ptr<4>(ni, ex);
    case 8: return directham_ptr<8>(ni, ex);
    case 16: return directham_ptr<16>(ni, ex);
    case 32: return directham_ptr<32>(ni, ex);
  }
  return nullptr;
}

}  // namespace gpamd
