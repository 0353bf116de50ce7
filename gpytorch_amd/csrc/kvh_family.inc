// Included by kvh_<family>.hip with GPAMD_KIND / GPAMD_NAME defined: the split-operand kernels of one covariance family
// (kv_gramh.hpp: generation AND contraction on the f16 matrix pipe).  CT = 1, 2 column tiles, with / without the extra
// VALU column.
#include "host.hpp"
#include "kv_gramh.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D>
const void* gramh_ptr(int ct, int ex, int ni) {
#define L(CT, EX, NI) \
  if (ct == CT && ex == EX && ni == NI) return reinterpret_cast<const void*>(&kv_gramh_kernel<GPAMD_KIND, D, CT, NI, EX>);
  L(2, 0, 2) L(2, 1, 2) L(1, 0, 1) L(1, 1, 1) L(2, 0, 1) L(2, 1, 1)
  if constexpr (D <= 16) { L(1, 0, 4) L(1, 1, 4) } else { L(1, 0, 2) L(1, 1, 2) }   // one column tile: four row tiles per wave up to 16 dimensions, two beyond (kgh_ni)
  // two column tiles x FOUR row tiles per wave ("lean": the operands of a half are fetched just before its MFMAs; kv_gramh.hpp): one Gram
  // MFMA per block (D <= 3) leaves the registers for it -- 90.2 vs 94.7 ms at n = 500 000, 65 columns, bitwise the same output
  if constexpr (GramF16<D>::KH == 1) {
    L(2, 0, 4)
    if constexpr (GPAMD_KIND == KIND_RBF) { L(2, 1, 4) }   // (with the extra column only the RBF fits without spilling more than one register)
  }
#undef L
  return nullptr;
}
}  // namespace

// d: valid dims (one of 1,2,3,4,5,6,8,10,12,16,20,24,32); ni: 32-row tiles per wave (kgh_ni(ct, d): 4 for one column tile, 2 for two -- 4 when d <= 3; 1 for small n)
const void* GPAMD_CAT(kvh_kernel_ptr_, GPAMD_NAME)(int d, int ct, int ex, int ni) {
  const void* fn = nullptr;
  with_dim(d, [&](auto D) { fn = gramh_ptr<D()>(ct, ex, ni); });
  return fn;
}

}  // namespace gpamd
