// Included by kvs_<family>.hip with GPAMD_KIND / GPAMD_NAME defined: the small-t Gram-form kernels (kv_gramv.hpp) of
// one covariance family.  A translation unit of their own because they are compiled with
// -mllvm -amdgpu-mfma-vgpr-form=1: their MFMA results are consumed by the VALU straight away (v_exp_f32), and the
// default AGPR destination costs one v_accvgpr_read per K element -- a quarter of the loop's VALU work.
#include "host.hpp"
#include "kv_gramv.hpp"

namespace gpamd {

#define GPAMD_CAT_(a, b) a##b
#define GPAMD_CAT(a, b) GPAMD_CAT_(a, b)

namespace {
template <int D>
const void* gramv_ptr(int tpad) {
#define L(T) \
  if (tpad == T) return reinterpret_cast<const void*>(&kv_gramv_kernel<GPAMD_KIND, D, T>);
  L(1) L(2) L(4) L(8) L(16)
#undef L
  return nullptr;
}
}  // namespace

// d: valid dims (one of 1,2,3,4,5,6,8,10,12,16,20,24,32); tpad: padded column count (1, 2, 4, 8, 16)
const void* GPAMD_CAT(kvs_kernel_ptr_, GPAMD_NAME)(int d, int tpad) {
  const void* fn = nullptr;
  with_dim(d, [&](auto D) { fn = gramv_ptr<D()>(tpad); });
  return fn;
}

}  // namespace gpamd
