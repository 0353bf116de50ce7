// Fused covariance MVM for WIDE inputs, 33 .. 512 dimensions, by DIRECT DIFFERENCES (RBF, Matern 1/2, 3/2, 5/2): the clouds kv_wide.hpp must refuse.
// kv_wide.hpp forms S = |z_i|^2 + |z_j|^2 - 2 z_j . z_i on the matrix pipe; its cancellation error grows with |z|^2, so the caller admits a cloud only
// within max |z|^2 <= 32 of the origin, and never Matern 1/2 (the cusp at S = 0).  Here S = sum_k (z_ik - z_jk)^2 is accumulated on the packed-f32
// vector pipe as kv_directh.hpp does it below 11 dimensions, with the number of dimensions a RUN-TIME loop over 16-dimension chunks: the error in S
// scales with |z_i - z_j|, not with |z|^2, and the diagonal of a symmetric product is exactly S = 0.  The reference has no such case distinction: its
// distances are one matmul of any width with a clamp (gpytorch/kernels/kernel.py:26-49); until now these clouds -- z-scored inputs at the default
// lengthscale from d = 40 or so on -- went through dense row blocks of K and a library GEMM (backend.kv_chunked).
//
// Everything behind the distances is kv_gramh.hpp's and kv_wide.hpp's: lane (h, i = l31) of a wave owns the 16 pairs (j(r, h), i), j(r, h) = (r & 3) +
// 8 (r >> 2) + 4 h, of a 32 x 32 block -- the B-operand slots of the contraction --, cov_pair_from_sq with 2^KGH_KSHIFT folded in, the hi/lo split of K,
// three v_mfma_f32_32x32x16_f16 per 16 contracted rows and column tile, the extra column on the VALU, vsplit_kernel's V planes and column multipliers
// (KvhArgs), the partial slabs, the done flag.  256 threads, 4 waves; a workgroup owns 128 NI output rows (wave w: rows 32 NI w ..) and one j chunk of
// the split-j plan.  The summation order is fixed: two calls give the same bits.
//
// Distance stage.  It reads the plain float32 prepared rows (gpamd_prep_points_f32: [n][dp], dp % 4 == 0, zero beyond d): no f16 image, no norms, no
// pre-pass -- a pre-stored [tile][chunk][k][j] order would replace the 8 ds_write_b32 per thread and chunk below by 2 ds_write_b128, against the 256
// ds_read_b128 per wave and chunk that bound the loop, so it would not pay for itself.  Per 128-row j tile and 16-dimension chunk:
//   * z_j: thread (row = tid / 2, half = tid % 2) loads dimensions 8 half .. + 7 of its row (two 16-byte loads) and stores them TRANSPOSED, Xf[k][j] with
//     a row stride of 132 floats -- the two halves of a wave land 32 banks apart: conflict-free --, so that ONE ds_read_b128 per dimension returns the
//     quad of consecutive rows j(4 q .. 4 q + 3, h): adjacent register pairs, the operands of v_pk_add_f32 / v_pk_fma_f32, the same address for the 32
//     lanes of a half-wave (broadcast).  Double-buffered: the global loads of chunk c + 1 (of chunk 0 of the next tile after the last) are issued before
//     the arithmetic of chunk c and stored behind it, one barrier per chunk;
//   * z_i: a lane reads the 16 values of ITS OWN row straight from global memory (four 16-byte loads per row tile and chunk, one chunk ahead, both
//     half-waves the same lines): they never cross lanes, so a round trip through LDS would only add to the traffic of the unit that bounds the loop;
//   * S: 64 NI accumulators per lane (4 j blocks x 16 pairs per row tile), per dimension and quad one packed subtraction and one packed multiply-add per
//     PAIR of adjacent j.
// Budget per wave and chunk: 256 ds_read_b128 (4 blocks x 4 quads x 16 dimensions, whatever NI) against 1024 NI packed VALU instructions.  A
// ds_read_b128 occupies the CU's LDS pipe for 8 cycles, a packed f32 instruction one SIMD for 4: per workgroup 4 x 256 x 8 = 8192 LDS cycles against
// 4096 NI VALU cycles on each of the four SIMDs.  NI = 1 is bound by LDS with the VALU half idle; NI = 2 balances the two (each z_j quad feeds two row
// tiles) and halves the LDS reads per pair -- the library instantiates NI = KWD_NI (below).  Wave-uniform z_j operands from scalar registers would take
// LDS out of the loop altogether, but the contraction's operand layout gives the two half-waves DIFFERENT rows j, so every instruction would compute
// one half in vain or the K words would have to be exchanged between the half-waves behind the covariance: not built.
// The covariance and the contraction follow per tile as in kv_wide.hpp, behind the last chunk: ~6 VALU + 2 transcendental instructions per pair and 6 CT
// MFMAs per block and row tile, against 2 d packed instructions per pair of pairs before it -- at d >= 33 the distances are the cost.
// Sizing: see KWD_NI.
#pragma once
#include "kv_wide.hpp"

namespace gpamd {

// 32-row tiles per wave of the instantiated kernels.  From -Rpass-analysis=kernel-resource-usage over the sixteen instantiations (the Makefile fails the
// build on scratch): NI = 2 takes 128 + 32 CT accumulators, 32 + 32 registers of z_i (this chunk, the next), 64 of z_j quads (two groups of 8 reads) and
// 8 + 16 CT of staging -- 256 VGPRs + 96 .. 193 AGPRs, no scratch, one wave per SIMD; LDS 16.5 KB of z_j chunks + 17 CT KB of V planes (+ 0.5 KB extra
// column): 34.3 KB (CT = 1), 51.7 KB (CT = 2).  NI = 1 would run two waves per SIMD, but <Matern 5/2, CT = 2, EX = 1> left 76 bytes of scratch per lane
// within 256 registers, and its loop is bound by LDS (above).
constexpr int KWD_NI = 2;
constexpr int KWD_LDJ = KW_TILE + 4;               // float row stride of the transposed z_j chunk (528 B: keeps 16-byte alignment, halves 32 banks apart)
constexpr int KWD_XB = KW_CHUNK * KWD_LDJ;         // floats of one z_j buffer
constexpr int kwd_waves(int ni) { return ni == 1 ? 2 : 1; }   // resident waves per SIMD the register allocator is held to

struct KvWideDirectArgs {
  KvhArgs h;   // a.X1 [n][dp], a.X2 [m][dp]: the prepared rows; Vt: only the extra column is read from it
  int dp;      // row stride in floats, a multiple of 4, zero beyond d
  int nc;      // chunks
};

template <int KIND, int CT, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kwd_waves(NI), kwd_waves(NI))))
void kv_wide_direct_kernel(KvWideDirectArgs wa) {
  static_assert(KIND == KIND_RBF || KIND == KIND_MATERN12 || KIND == KIND_MATERN32 || KIND == KIND_MATERN52, "RBF, Matern 1/2, 3/2, 5/2");
  static_assert((CT == 1 || CT == 2) && (NI == 1 || NI == 2), "one or two column tiles, one or two row tiles per wave");
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int BN = KGH_BN, LDH = KGH_LDH, TC = 32 * CT, JB = BN / 32;
  constexpr int LDJ = KWD_LDJ, XB = KWD_XB, KC = KW_CHUNK;
  constexpr int VQ = TC * (BN / 8) / NT;       // 16-byte pieces per thread and V plane
  static_assert(BN == KW_TILE && NT == 2 * BN, "two threads stage one row of the j tile");
  const KvhArgs& ka = wa.h;
  const KvArgs& a = ka.a;
  __shared__ __attribute__((aligned(16))) _Float16 Vhs[TC * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 Vls[TC * LDH];
  __shared__ __attribute__((aligned(16))) float Xf[2 * XB];   // [buf][k][j]
  __shared__ __attribute__((aligned(16))) float Es[EX ? BN : 4];

  if (a.done && *a.done) return;
  float negone;   // -1.0f the optimiser cannot see through (the lo word below; kv_gramh_body.inc gen_b)
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(negone));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;                  // multiple of BN
  const int jend = min(a.m, jbeg + a.jchunk);
  const int ibase = rb * (NW * NI * 32) + wave * (NI * 32);
  const int nc = wa.nc, dp = wa.dp;

  f32x16 acc[NI][CT];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ni][ct][r] = 0.f;
  f32x2 eacc2[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) eacc2[ni] = (f32x2)(0.f);

  // chunk c of this lane's own rows (a row beyond n repeats the last one: never written) and of the j tile starting at j0: global -> registers
  const float* xi[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) xi[ni] = a.X1 + (int64_t)min(ibase + ni * 32 + l31, a.n - 1) * dp;
  const int jr = tid >> 1, hh = tid & 1;
  f32x4 zin[NI][KC / 4], pj[2];
  auto load_z = [&](int j0, int c) {
    const int k0 = KC * c;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int g = 0; g < KC / 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k0 + 4 * g < dp) v = *reinterpret_cast<const f32x4*>(xi[ni] + k0 + 4 * g);
        zin[ni][g] = v;
      }
    const int j = j0 + jr;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};   // rows beyond jend, dimensions beyond dp: zero (K stays finite against V = 0)
      if (j < jend && k0 + 8 * hh + 4 * g < dp) v = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * dp + k0 + 8 * hh + 4 * g);
      pj[g] = v;
    }
  };
  auto store_zj = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 8; ++e) Xf[buf * XB + (8 * hh + e) * LDJ + jr] = pj[e >> 2][e & 3];
  };
  // V planes and extra column of the tile starting at j0 (rows beyond jend: zero planes, zero extra column)
  u32x4 pvh[VQ], pvl[VQ];
  f32x4 pe = {0.f, 0.f, 0.f, 0.f};
  auto load_v = [&](int j0) {
    const int64_t jc = min((int64_t)j0, ka.ldh - BN);
#pragma unroll
    for (int rr = 0; rr < VQ; ++rr) {
      const int idx = tid + NT * rr;
      const int c = idx / (BN / 8), q = idx % (BN / 8);
      const int64_t off = (int64_t)c * ka.ldh + jc + 8 * q;
      pvh[rr] = *reinterpret_cast<const u32x4*>(ka.Vh + off);
      pvl[rr] = *reinterpret_cast<const u32x4*>(ka.Vl + off);
    }
    if constexpr (EX) {
      if (tid >= BN && tid < BN + BN / 4) {
        const int j = j0 + 4 * (tid - BN);
        const float* src = a.Vt + (int64_t)TC * a.ldv + j;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j + 4 <= jend) {
          v = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < jend) v[e] = src[e];
        }
        pe = v;
      }
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int rr = 0; rr < VQ; ++rr) {
      const int idx = tid + NT * rr;
      const int c = idx / (BN / 8), q = idx % (BN / 8);
      *reinterpret_cast<u32x4*>(&Vhs[c * LDH + 8 * q]) = pvh[rr];
      *reinterpret_cast<u32x4*>(&Vls[c * LDH + 8 * q]) = pvl[rr];
    }
    if constexpr (EX) {
      if (tid >= BN && tid < BN + BN / 4) *reinterpret_cast<f32x4*>(&Es[4 * (tid - BN)]) = pe;
    }
  };

  load_z(jbeg, 0);
  load_v(jbeg);
  store_zj(0);
  store_v();
  __syncthreads();

  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    const bool more_tiles = j0 + BN < jend;
    // S of the pairs (j(r, h) of block jb, i): sq[ni][jb][r]
    f32x16 sq[NI][JB];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sq[ni][jb][r] = 0.f;

#pragma unroll 1
    for (int c = 0; c < nc; ++c, buf ^= 1) {
      const bool last = c == nc - 1;
      f32x4 zi[NI][KC / 4];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int g = 0; g < KC / 4; ++g) zi[ni][g] = zin[ni][g];
      // (after the last chunk of the last tile: the lane's chunk 0 again and an all-zero tile, never used)
      load_z(last ? j0 + BN : j0, last ? 0 : c + 1);
      // A group = the quad of rows j(4 q .. 4 q + 3, h) of block jb (g = 4 jb + q), one half of the chunk's dimensions: KG reads, 4 KG NI packed
      // instructions.  The reads of group u + 1 are issued before the arithmetic of group u and sched_barrier pins that order -- left to itself the
      // scheduler hoists all 256 reads of a chunk (3 KB of scratch per lane)
      const float* xb = Xf + buf * XB + 4 * h;
      constexpr int KG = 8, NG = 4 * JB * (KC / KG);
      f32x4 zq[2][KG];
      auto read_group = [&](int u, f32x4* dst) {
        const int g = u / (KC / KG), kh = u % (KC / KG);
#pragma unroll
        for (int k = 0; k < KG; ++k) dst[k] = *reinterpret_cast<const f32x4*>(xb + (KG * kh + k) * LDJ + 8 * g);   // (32 jb + 8 q = 8 g)
      };
      read_group(0, zq[0]);
#pragma unroll
      for (int u = 0; u < NG; ++u) {
        if (u + 1 < NG) read_group(u + 1, zq[(u + 1) & 1]);
        asm volatile("" ::: "memory");   // (the optimiser's passes before the scheduler: no read of a later group moves up past here)
        const int g = u / (KC / KG), kh = u % (KC / KG), jb = g >> 2, q = g & 3;
#pragma unroll
        for (int k = 0; k < KG; ++k) {
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const f32x2 z = (f32x2)(zi[ni][(KG * kh + k) >> 2][k & 3]);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const f32x2 df = z - (f32x2){zq[u & 1][k][2 * p], zq[u & 1][k][2 * p + 1]};
              f32x2 sv = {sq[ni][jb][4 * q + 2 * p], sq[ni][jb][4 * q + 2 * p + 1]};
              sv = __builtin_elementwise_fma(df, df, sv);
              sq[ni][jb][4 * q + 2 * p] = sv[0];
              sq[ni][jb][4 * q + 2 * p + 1] = sv[1];
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // unconditional (after the last chunk of the last tile: zero rows nobody reads) -- behind a branch the optimiser sinks the whole arithmetic of the
      // chunk past it, away from its reads
      store_zj(buf ^ 1);
      __syncthreads();   // chunk c + 1 is staged; every wave is done with this buffer
    }

    if (more_tiles) load_v(j0 + BN);

    // generation and contraction (kv_wide.hpp): lane (l31, h) holds S[j(r, h)][i = l31] -- its own B operands of the contraction
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      __builtin_amdgcn_sched_barrier(0);   // the operand reads of a block stay in it
      f16x8 vh[2][CT], vl[2][CT];
#pragma unroll
      for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int o = (ct * 32 + l31) * LDH + jb * 32 + 16 * mf + 8 * h;
          vh[mf][ct] = *reinterpret_cast<const f16x8*>(&Vhs[o]);
          vl[mf][ct] = *reinterpret_cast<const f16x8*>(&Vls[o]);
        }
#pragma unroll
      for (int mf = 0; mf < 2; ++mf) {
        f32x4 ev[2];
        if constexpr (EX) {
#pragma unroll
          for (int g = 0; g < 2; ++g) ev[g] = *reinterpret_cast<const f32x4*>(&Es[jb * 32 + 16 * mf + 8 * g + 4 * h]);
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          u32x4 kh, kl;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const f32x2 s2 = {sq[ni][jb][8 * mf + 2 * p], sq[ni][jb][8 * mf + 2 * p + 1]};
            const f32x2 kv = cov_pair_from_sq<KIND>(s2, 0.f, (float)KGH_KSHIFT);
            if constexpr (EX) {
              const f32x2 e2 = {ev[p >> 1][2 * (p & 1)], ev[p >> 1][2 * (p & 1) + 1]};
              eacc2[ni] = __builtin_elementwise_fma(kv, e2, eacc2[ni]);
            }
            // hi rounded toward zero, lo = K - hi from one v_fma_mix_f32 per element (f32 denormals flushed: the unit's build flag)
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            const uint32_t hiw = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(kv[0], kv[1]));
            const f16x2 hv = __builtin_bit_cast(f16x2, hiw);
            const float l0 = __builtin_fmaf((float)hv[0], negone, kv[0]);
            const float l1 = __builtin_fmaf((float)hv[1], negone, kv[1]);
            kh[p] = hiw;
            kl[p] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(l0, l1));
          }
          const f16x8 khv = __builtin_bit_cast(f16x8, kh);
          const f16x8 klv = __builtin_bit_cast(f16x8, kl);
          // Vl Kh, Vh Kl, then the leading Vh Kh; consecutive instructions alternate accumulators
#pragma unroll
          for (int q = 0; q < 3 * CT; ++q) {
            const int ct = q % CT, term = q / CT;
            acc[ni][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 0 ? vl[mf][ct] : vh[mf][ct], term == 1 ? klv : khv, acc[ni][ct], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();   // every wave is done with the V planes and the extra column of this tile
    if (more_tiles) store_v();   // (visible to every wave behind the barriers of the next tile's chunk loop)
  }

  mfma_result_fence();   // the accumulators of the last contraction MFMAs are read next (common.hpp; once per workgroup)
  float* Pout = a.P + (int64_t)s * a.pstride;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int i = ibase + ni * 32 + l31;
    if (i < a.n) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (c < a.t) Pout[(int64_t)c * a.ldo + i] = acc[ni][ct][r] * ka.colmul[c];
        }
    }
    if constexpr (EX) {
      const float part = eacc2[ni][0] + eacc2[ni][1];
      const float tot = part + __shfl_xor(part, 32, 64);
      if (h == 0 && i < a.n) Pout[(int64_t)TC * a.ldo + i] = tot * ka.colmul[TC];
    }
  }
}

}  // namespace gpamd
