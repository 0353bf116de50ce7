// Included by kvp_<a>_<b>.hip with GPAMD_KA / GPAMD_KB / GPAMD_NAME defined: the product kernels of one pair of factor families (kv_directp.hpp), for
// every (D_A, D_B) in 1..3 x 1..3 the code rule admits (equal families: D_A <= D_B), NI = 1, 2 row tiles per wave, without / with the extra VALU column.
#include "host.hpp"
#include "kv_directp.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int DA, int DB>
const void* directp_ptr(int ni, int ex) {
  if constexpr (GPAMD_KA != GPAMD_KB || DA <= DB) {
#define KDP_CASE(N, E) if (ni == N && ex == E) return reinterpret_cast<const void*>(&kv_directp_kernel<GPAMD_KA, GPAMD_KB, DA, DB, N, E>);
    KDP_CASE(1, 0) KDP_CASE(1, 1) KDP_CASE(2, 0) KDP_CASE(2, 1)
#undef KDP_CASE
  }
  return nullptr;
}
}  // namespace

// da, db: columns of the two factors (1..3); ni: 32-row tiles per wave; ex: extra VALU column
const void* GPAMD_CAT(kvp_kernel_ptr_, GPAMD_NAME)(int da, int db, int ni, int ex) {
  switch (4 * da + db) {
    case 5: return directp_ptr<1, 1>(ni, ex);
    case 6: return directp_ptr<1, 2>(ni, ex);
    case 7: return directp_ptr<1, 3>(ni, ex);
    case 9: return directp_ptr<2, 1>(ni, ex);
    case 10: return directp_ptr<2, 2>(ni, ex);
    case 11: return directp_ptr<2, 3>(ni, ex);
    case 13: return directp_ptr<3, 1>(ni, ex);
    case 14: return directp_ptr<3, 2>(ni, ex);
    case 15: return directp_ptr<3, 3>(ni, ex);
  }
  return nullptr;
}

}  // namespace gpamd
