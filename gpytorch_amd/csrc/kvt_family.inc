// Included by kvt_<base>.hip with GPAMD_KB / GPAMD_NAME defined: the product-structure (tensor-product Matern) kernels of one base family
// (kv_directps.hpp), for d = 2 .. 8, NI = 1, 2 row tiles per wave, without / with the extra VALU column.
#include "host.hpp"
#include "kv_directps.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D>
const void* directps_ptr(int ni, int ex) {
#define KPS_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directps_kernel<GPAMD_KB, D, N, E>);
  KPS_CASE(1, 0) KPS_CASE(1, 1) KPS_CASE(2, 0) KPS_CASE(2, 1)
#undef KPS_CASE
  return nullptr;
}
}  // namespace

// d: input dimensions (2..8); ni: 32-row tiles per wave; ex: extra VALU column
const void* GPAMD_CAT(kvt_kernel_ptr_, GPAMD_NAME)(int d, int ni, int ex) {
  switch (d) {
    case 2: return directps_ptr<2>(ni, ex);
    case 3: return directps_ptr<3>(ni, ex);
    case 4: return directps_ptr<4>(ni, ex);
    case 5: return directps_ptr<5>(ni, ex);
    case 6: return directps_ptr<6>(ni, ex);
    case 7: return directps_ptr<7>(ni, ex);
    case 8: return directps_ptr<8>(ni, ex);
  }
  return nullptr;
}

}  // namespace gpamd
