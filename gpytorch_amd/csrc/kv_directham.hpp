// Fused covariance MVM of the HAMMING family (KIND_HAMMING): the inverse-multiquadric Hamming covariance over fixed-length one-hot encoded sequences of
// gpytorch/kernels/hamming_kernel.py:130-160 (whose hamming_dist broadcasts an n x m x T x V tensor),
//     k(x, x') = ((1 + alpha) / (alpha + c))^beta = k0 (1 + c / alpha)^(-beta),   c = the Hamming distance in 0..T,   k0 = ((1 + alpha) / alpha)^beta.
// The kernel generates k~ = (1 + c / alpha)^(-beta) in (0, 1] with an exact unit diagonal (the caller's scale carries k0), which IS the RQ family's
// radial function at s = c / alpha with shape beta (cov_pair_from_sq<KIND_RQ>: one v_log_f32, one v_exp_f32 per element).  What is new is where s
// comes from: INTEGER instructions on packed tokens.
//
// The prepared row (families.hamming_prep is the one place that writes it): one BYTE per position, token + 1, four positions per dword, padded with
// the byte 1 up to the instantiated width W dwords (W = 4, 8, 16, 32 for T <= 16, 32, 64, 128), carried as float32 [n, W].  Bytes lie in 1..127, so
//   - every dword is a normal, finite float bit pattern (exponent field 2 b3 + (b2 >> 7) in 2..254): loads, LDS staging and register moves keep its bits
//     whatever the denormal mode -- no arithmetic ever touches it as a float;
//   - the number of positions in which two dwords differ is popcount(((a ^ b) + 0x7f7f7f7f) & 0x80808080): a byte of a ^ b is in 0..127, so adding
//     0x7f sets its top bit exactly when it is non-zero and never carries into the next byte.
// Per dword and element: v_xor, v_add (one v_xad_u32 where the compiler fuses them), v_and, v_bcnt_u32_b32 with the running count as its addend.  Equal
// padding contributes nothing; a row of zeros (the tile rows past the end of a chunk) differs from a valid row in every byte: c = 4 W, finite.
//
// It IS kv_directh_kernel's body (kv_directh_body.inc) with ONE 32-column tile and a LAZY functor, as kv_directgibbs.hpp and kv_directsm.hpp.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KHM_COLS = 32;            // columns per launch group (+ 1 extra VALU column): one tile, K regenerated per group
constexpr int KHM_MAX_POSITIONS = 128;  // sequence length T
constexpr int KHM_CHUNK = 8;            // dwords of a row whose reads are in flight at a time (DirectHamming::pair_rows)
constexpr bool khm_width_ok(int width) { return width == 4 || width == 8 || width == 16 || width == 32; }   // the prepared width in dwords
constexpr bool khm_param_ok(float v) { return v > 0.f && v <= 3.402823466e38f; }   // 1 / alpha, beta: positive and finite (NaN fails the first test)
// 32-row tiles per wave: two, or one for few output rows (the rule of the Gibbs kernels, whose plan the family borrows: api.hip)
constexpr int khm_ni(bool small, int) { return small ? 1 : 2; }

struct KvHamArgs : KvhArgs {
  float inv_alpha, beta;   // 1 / alpha and beta of k~ = (1 + c / alpha)^(-beta)
};

// The bits of one packed dword.  Its argument is a float BY VALUE: __builtin_bit_cast applied to an element of an ext_vector (r[1], v[e]) reinterprets
// the vector object from its first byte, i.e. returns element 0 whatever the index -- every element goes through this function instead
__device__ __forceinline__ uint32_t ham_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// acc + the number of byte positions in which the packed dwords a and b differ (bytes in 0..127: see above)
__device__ __forceinline__ uint32_t ham_mismatch(float a, float b, uint32_t acc) {
  return (uint32_t)__builtin_popcount(((ham_bits(a) ^ ham_bits(b)) + 0x7f7f7f7fu) & 0x80808080u) + acc;
}

template <int W>
struct DirectHamming {
  static_assert(khm_width_ok(W), "prepared width 4, 8, 16 or 32 dwords (T <= 16, 32, 64, 128)");
  static constexpr int SPLIT = W;
  static constexpr bool LAZY = true;
  struct Shape {
    float inv_alpha, beta;
  };
  static __device__ __forceinline__ Shape shape(const KvHamArgs& ka) { return Shape{pp_uniform(ka.inv_alpha), pp_uniform(ka.beta)}; }   // scalar registers
  template <typename R>
  static __device__ __forceinline__ f32x2 pair_rows(const float* zi, R row, const Shape& sh) {
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int k0 = 0; k0 < W; k0 += KHM_CHUNK) {
#pragma unroll
      for (int k = k0; k < k0 + KHM_CHUNK && k < W; ++k) {
        const f32x2 r = row(k);
        c0 = ham_mismatch(zi[k], r[0], c0);
        c1 = ham_mismatch(zi[k], r[1], c1);
      }
      if constexpr (W > KHM_CHUNK) {
        // a row is up to 32 dwords wide: one chunk's column reads are in flight at a time, and its counts are COMPUTED here -- the tie (a volatile
        // asm keeps its place among the barriers) stops the compiler from sinking the integer work below later reads, which left every column of
        // a half live at once and spilled them at W = 32; the sched_barrier stops the scheduler from hoisting the next chunk's reads above it
        // (kv_directsm.hpp does the same per input dimension)
        mfma_tie(c0);
        mfma_tie(c1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const f32x2 s = (f32x2){(float)c0, (float)c1} * sh.inv_alpha;
    return cov_pair_from_sq<KIND_RQ>(s, sh.beta, (float)KGH_KSHIFT);   // c = 0: log2(1) = 0, exp2(KSHIFT) exactly
  }
};

// Same launch bounds and waves_per_eu for every width (those of kv_directgibbs_kernel)
template <int W, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_directham_kernel(KvHamArgs ka) {
  using GEN = DirectHamming<W>;
  constexpr int D = W, CT = 1;
#include "kv_directh_body.inc"
}

}  // namespace gpamd
