// The split-operand instantiations of the fused bilinear-derivative kernel (kv_grad2.hpp, WSPLIT = 1) in a translation unit of their own
// (build parallelism); launched by kvm_grad2.hip.  A kvm_* unit: compiled with -mllvm -amdgpu-mfma-vgpr-form=1.
#include "kv_grad2_host.hpp"

namespace gpamd {

bool grad2_launch_split(int kind, int dk, int mode, const Grad2Args& a, unsigned grid, hipStream_t st) {
  return grad2_launch<1>(kind, dk, mode, a, grid, st);
}

}  // namespace gpamd
