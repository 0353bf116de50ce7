// Host launch of the fused bilinear-derivative kernel (kv_grad2.hpp), shared by kvm_grad2.hip (WSPLIT = 0) and kvm_grad3.hip (WSPLIT = 1: the
// split-operand contraction, a translation unit of its own for build parallelism).
#pragma once
#include "host.hpp"
#include "kv_grad2.hpp"

namespace gpamd {

// dynamic LDS: the W^T / distance tiles (WSPLIT: the two staged R planes) + the Gram operands + (mode 1) the per-dimension staging
template <int D, int WSPLIT>
size_t grad2_lds(int rs, int mode) {
  constexpr int KH = GramF16<D>::KH;
  constexpr int GZ = (1 + 2 * D + 3) / 4;
  const size_t wt = WSPLIT ? (size_t)2 * G2_BN * G2_CPL * 2 : (size_t)(4 * 32 + G2_BN) * rs * 4;
  return wt + (size_t)KH * G2_BN * 16 * 2 + (mode ? (size_t)4 * GZ * (G2_BN + 4) * 4 : 0);
}

// kind: GPAMD_* (a Gram-form family); dk: kernel dims; mode 0: one lengthscale sum, 1: per-dimension sums / input gradients (up to 16
// dimensions: beyond, the caller's row-block path, backend.kv_grad_generic).  false: no instantiation
template <int WSPLIT>
bool grad2_launch(int kind, int dk, int mode, const Grad2Args& a, unsigned grid, hipStream_t st) {
  bool launched = false;
  with_kind<KINDS_GRAM>(kind, [&](auto K) {
    constexpr int KIND = decltype(K)::value;
    with_dim(dk, [&](auto DK) {
      constexpr int D = decltype(DK)::value;
      const size_t lds = grad2_lds<D, WSPLIT>(a.rs, mode);
      auto launch = [&](auto kfn) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
        launched = true;
      };
      if (mode == 0) launch(kv_grad2_kernel<KIND, D, 0, WSPLIT>);
      else if constexpr (D <= 16) launch(kv_grad2_kernel<KIND, D, 1, WSPLIT>);
    });
  });
  return launched;
}

bool grad2_launch_split(int kind, int dk, int mode, const Grad2Args& a, unsigned grid, hipStream_t st);   // kvm_grad3.hip: grad2_launch<1>

}  // namespace gpamd
