// Included by kvm_<family>.hip with GPAMD_KIND / GPAMD_NAME defined: the 5..24-column Gram-form kernels of one covariance
// family -- contraction on a 16-column tile (kv_gram16.hpp, v_mfma_f32_16x16x1_4B_f32) or in column groups of four
// (kv_gram4.hpp, v_mfma_f32_4x4x1_16B_f32).  Compiled like kvs_<family>.hip with
// -mllvm -amdgpu-mfma-vgpr-form=1 (the Gram MFMA results are consumed by v_exp_f32 straight away).
#include "host.hpp"
#include "kv_gram16.hpp"
#include "kv_gram4.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D>
const void* gram4_ptr(int groups) {
#define L(G) \
  if (groups == G) return reinterpret_cast<const void*>(&kv_gram4_kernel<GPAMD_KIND, D, G>);
  L(2) L(3) L(6)
#undef L
  if (groups == 16) return reinterpret_cast<const void*>(&kv_gram16_kernel<GPAMD_KIND, D, 0>);
  if (groups == 17) return reinterpret_cast<const void*>(&kv_gram16_kernel<GPAMD_KIND, D, 1>);
  return nullptr;
}
}  // namespace

// d: valid dims (one of 1,2,3,4,5,6,8,10,12,16); groups: column groups of four (2, 3, 6) of kv_gram4, or 16 / 17 = the
// 16-column tile kernel kv_gram16 without / with the extra VALU column
const void* GPAMD_CAT(kvm_kernel_ptr_, GPAMD_NAME)(int d, int groups) {
  const void* fn = nullptr;
  with_dim<16>(d, [&](auto D) { fn = gram4_ptr<D()>(groups); });
  return fn;
}

}  // namespace gpamd
