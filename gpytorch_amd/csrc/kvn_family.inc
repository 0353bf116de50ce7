// Included by kvn_<base>.hip with GPAMD_KB / GPAMD_NAME defined: the Newton-Girard additive kernels of one base family (kv_directng.hpp), for d = 2 .. 8,
// the degree caps min(d, 3) and d, NI = 1, 2 row tiles per wave, without / with the extra VALU column.
#include "host.hpp"
#include "kv_directng.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D, int RC>
const void* directng_ptr(int ni, int ex) {
#define KNG_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directng_kernel<GPAMD_KB, D, RC, N, E>);
  KNG_CASE(1, 0) KNG_CASE(1, 1) KNG_CASE(2, 0) KNG_CASE(2, 1)
#undef KNG_CASE
  return nullptr;
}
template <int D>
const void* directng_cap(int full, int ni, int ex) {
  return full ? directng_ptr<D, D>(ni, ex) : directng_ptr<D, ng_cap(D, 1)>(ni, ex);
}
}  // namespace

// d: input dimensions (2..8); full: degree cap d (else min(d, 3)); ni: 32-row tiles per wave; ex: extra VALU column
const void* GPAMD_CAT(kvn_kernel_ptr_, GPAMD_NAME)(int d, int full, int ni, int ex) {
  switch (d) {
    case 2: return directng_cap<2>(full, ni, ex);
    case 3: return directng_cap<3>(full, ni, ex);
    case 4: return directng_cap<4>(full, ni, ex);
    case 5: return directng_cap<5>(full, ni, ex);
    case 6: return directng_cap<6>(full, ni, ex);
    case 7: return directng_cap<7>(full, ni, ex);
    case 8: return directng_cap<8>(full, ni, ex);
  }
  return nullptr;
}

}  // namespace gpamd
