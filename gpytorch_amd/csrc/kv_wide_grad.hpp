// Fused bilinear derivative for WIDE inputs, 33 .. 512 dimensions (RBF, Matern 3/2, 5/2): the derivative kernel of kv_wide.hpp.
//
//   g[0] = sum_ij W_ij k_ij,   g[1 + q] = sum_ij A_ij (z_iq - z_jq)^2,   Gz1[i] = 2 (z_i sum_j A_ij - sum_j A_ij z_j),   W = L^T R,  A = W o dk/ds
//
// the contract of kv_grad2.hpp (LinearOperator._bilinear_derivative on the kernel operator + the dense backward of
// gpytorch/functions/rbf_covariance.py:26-29, matern_covariance.py:53-56; input gradients as the KeOps precedent provides them), which stops at 16
// dimensions; until now such clouds formed W as dense row blocks with a library GEMM (backend.kv_grad_generic) and had no input gradients at all.
//
// Squared distances are kv_wide_kernel's: the split image of wide_split_kernel, a run-time loop over 16-dimension chunks of z_j . z_i on
// v_mfma_f32_32x32x16_f16 (hi.hi, hi.lo, lo.hi), double-buffered LDS, f32 norms on the VALU, the clamp at 0.  256 threads, 4 waves; a workgroup owns
// 128 output rows (wave w: rows 32 w ..) and one j chunk of a split-j plan, the j tile is 128 rows.  Per j tile, behind the chunk loop:
//   * W tile.  W_ij = sum_c L_ci R_cj on v_mfma_f32_32x32x2_f32 with R as the A operand (rows j) and L as the B operand (rows i): the result has the
//     lane layout of the distance tile -- lane (i = l31, h), register r <-> j = (r & 3) + 8 (r >> 2) + 4 h -- so S, k, dk/ds and W meet in one slot.
//     The L tile [t][128] of the row block is staged in LDS once, the R tile [t][128] once per j tile; in MODE 0 two 32-row j blocks run interleaved.  Plain f32
//     products: exact to f32 rounding for every t, none of the round-down bias of the f16 pipe (kv_wsplit.hpp), hence no row / block signs.  The
//     price is 64 cycles per two columns and 32 x 32 block: at 65 columns 2112 cycles where a split-W form would take 480.  NOT BUILT: the split-W
//     variant.  Up to KWG_MAXT = 66 columns per pass; more columns run as further passes whose sums add (g is linear in W), each regenerating S.
//   * MODE 0 (one lengthscale, no input gradients): sum W k and sum A S on the VALU, per lane in f32 per tile, across tiles in float64.  No
//     per-dimension work at all.
//   * MODE 1 (per-dimension sums, optionally Gz1): A sc (sc: a power of two from max|L_c| max|R_c|, so that |A sc| <= 2^12) is split into hi/lo f16 as
//     kv_wide_kernel splits K and stays in registers (64 per lane) as the B operand of a SECOND contraction over j, the forward's K.V with the cloud
//     itself as V:   u_iq = sum_j A_ij z_jq,   v_iq = sum_j A_ij z_jq^2   (the [z | z^2] columns of kv_grad2.hpp), 3 MFMAs per 16 contracted rows.
//     It needs z_j with j as the k index: the TRANSPOSED split image of wide_split_t_kernel (once per prepared cloud, cached beside the image) -- per
//     j tile and 32-dimension block the hi/lo planes of z and of z^2 as [dimension][128 positions] in the permuted k-slot order of the V planes
//     (kv_vsplit.hpp), 16 KB per (z | z^2) pair, staged double-buffered through the LDS of the z chunks, which are dead by then.
//     The accumulators are row-resident, [q(r, h)][i = l31] as the forward's: 16 registers per 32 dimensions and quantity.  A workgroup therefore
//     covers KWG_DB = 64 dimensions (64 accumulator registers: u and v of two 32-dimension blocks) and the dimension blocks run on grid axis y,
//     EACH REGENERATING S AND W: d = 512 costs eight times the Gram work of the single-lengthscale mode.  That is the price of one orientation for
//     both the per-dimension sums and Gz1 (which needs u row-resident); 128 dimensions per block did not fit 256 registers beside the 64 of the A
//     operands.  Row sums rs_i = sum_j A_ij come from the VALU (f32 per tile, float64 across tiles).
//     Epilogue: per dimension  sum_i [z_iq^2 rs_i - 2 z_iq u_iq + v_iq]  is combined in float64 from the f32 accumulators, reduced over the 128 rows in
//     float64; u and rs go to per-slab workspaces and wide_gz_reduce_kernel forms 2 (z_iq rs_i - u_iq) in float64.
// No atomics: partials per (pass, slab, row block[, dimension block]) in a workspace, summed in a fixed order by the reduce kernels -- two calls
// give the same bits.  Rows beyond n / m: the staged L / R tiles are zero there, so W = 0 against finite k (the image rows are zero too).
// Sizing (from -Rpass-analysis=kernel-resource-usage; the Makefile fails the build on scratch).  MODE 0: 196 VGPRs, two waves per SIMD.  MODE 1 held to
// two waves per SIMD left 56 .. 136 bytes of scratch per lane (64 accumulator + 64 operand + 64 distance registers): it is built for ONE wave per
// SIMD, where a pass of more than 44 columns puts it anyway -- LDS is 34.5 KB + 1 KB per two columns: 46 KB at 11 columns, 101 KB at 65.
#pragma once
#include "kv_wide.hpp"

namespace gpamd {

constexpr int KWG_DB = 64;                      // dimensions per workgroup in the per-dimension mode
constexpr int KWG_MAXT = 66;                    // columns per pass
constexpr int KWG_TBUF = 2 * 32 * KGH_LDH;      // f16 elements of one staged (hi, lo) plane pair of 32 dimensions
constexpr int KWG_TBLK = 2 * 32 * KGH_BN;       // ... of the same pair in the transposed image
constexpr int KWG_UNION = 2 * KWG_TBUF * 2;     // bytes: two plane-pair buffers >= the two z-chunk buffers of the distance loop
static_assert(KWG_UNION >= 2 * 2 * KW_TCH * 2, "the plane buffers reuse the LDS of the z chunks");
constexpr int KWG_ASHIFT = 12;                  // |A sc| <= 2^12
constexpr int kwg_dblocks(int d) { return (d + KWG_DB - 1) / KWG_DB; }
constexpr int kwg_waves(int mode) { return mode ? 1 : 2; }   // resident waves per SIMD the register allocator is held to (header: Sizing)
constexpr size_t kwg_lds(int tpad) { return (size_t)KWG_UNION + KGH_BN * 4 + (size_t)2 * tpad * KGH_BN * 4; }

struct KvWideGradArgs {
  const _Float16* Z1;     // split images (kv_wide.hpp)
  const _Float16* Z2;
  const _Float16* T2;     // transposed image of the contracted cloud: [tiles][dblocks][4][KWG_TBLK] (MODE 1)
  const float* N1;
  const float* N2;
  const float* X1;        // [n][dp] prepared rows (epilogue of MODE 1)
  const float* Lt;        // [tp][ldl], [tp][ldr]: the columns of this pass
  const float* Rt;
  int64_t ldl, ldr;
  int n, m, dp, nc, tp, tpad;
  int S, jchunk, nrb;
  const float* wscale;    // [2]: sc, 1 / sc
  double* part;           // [nrb S][pstride]: MODE 0 (sum W k, sum A S); MODE 1 (sum W k | sc * per-dimension sums of every block)
  int pstride;
  float* U;               // optional [S][n][dq] sc u, [S][n] sc rs (input gradients) or nullptr
  float* RS;
  int dq;
};

template <int KIND>
__device__ __forceinline__ void wide_cov_dcov(float s, float& k, float& dk) {
  if constexpr (KIND == KIND_RBF) {
    k = __builtin_amdgcn_exp2f(-s);
    dk = -0.6931471805599453f * k;
  } else {
    const float r = __builtin_amdgcn_sqrtf(s);
    const float e = __builtin_amdgcn_exp2f(-r * 1.4426950408889634f);
    if constexpr (KIND == KIND_MATERN32) {
      k = (1.0f + r) * e;
      dk = -0.5f * e;
    } else {
      k = __builtin_fmaf(s, 1.0f / 3.0f, 1.0f + r) * e;
      dk = -(1.0f + r) * e * (1.0f / 6.0f);
    }
  }
}

// ---- pre-pass.  Grid (tiles, 32-dimension blocks), 256 threads: thread (dimension, 8 positions) x 2.  position 16 g + 8 h + e of a tile holds row
// 16 g + (e & 3) + 8 (e >> 2) + 4 h (kv_vsplit.hpp); z is the STORED operand hi + lo of the image, z^2 its f32 square.  Zero beyond n and beyond d
__global__ __launch_bounds__(256) void wide_split_t_kernel(const float* __restrict__ Xp, int n, int d, int dp, _Float16* __restrict__ T) {
  const int tile = blockIdx.x, blk = blockIdx.y;
  _Float16* base = T + ((int64_t)tile * gridDim.y + blk) * (2 * KWG_TBLK);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = threadIdx.x + 256 * it;
    const int row = idx & 31, pos8 = idx >> 5;
    const int q = blk * 32 + row;
    const int ja = 16 * (pos8 >> 1) + 4 * (pos8 & 1);
    f16x8 zh, zl, sh, sl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = tile * KW_TILE + (e < 4 ? ja : ja + 8) + (e & 3);
      const float z = (j < n && q < d) ? Xp[(int64_t)j * dp + q] : 0.f;
      _Float16 a, b;
      f16_split(z, a, b);
      zh[e] = a;
      zl[e] = b;
      const float zz = (float)a + (float)b;
      f16_split(zz * zz, a, b);
      sh[e] = a;
      sl[e] = b;
    }
    _Float16* dst = base + row * KGH_BN + pos8 * 8;
    *reinterpret_cast<f16x8*>(dst) = zh;
    *reinterpret_cast<f16x8*>(dst + 32 * KGH_BN) = zl;
    *reinterpret_cast<f16x8*>(dst + KWG_TBLK) = sh;
    *reinterpret_cast<f16x8*>(dst + KWG_TBLK + 32 * KGH_BN) = sl;
  }
}

template <int KIND, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kwg_waves(MODE), kwg_waves(MODE))))
void kv_wide_grad_kernel(KvWideGradArgs a) {
  static_assert(KIND == KIND_RBF || KIND == KIND_MATERN32 || KIND == KIND_MATERN52, "RBF, Matern 3/2, 5/2");
  constexpr int NT = 256, BN = KGH_BN, LDH = KGH_LDH, JB = BN / 32;
  constexpr int ZB = 2 * KW_TCH;               // f16 elements of one z staging buffer: the z_i tile-chunk, then the z_j tile-chunk
  constexpr int NRED = MODE ? 1 + KWG_DB : 2;
  constexpr int NQ = MODE ? 1 : 2;             // 32-row j blocks whose W tiles run interleaved (MODE 1: its registers hold one)
  extern __shared__ __attribute__((aligned(16))) unsigned char kwg_dyn[];
  _Float16* Zs = reinterpret_cast<_Float16*>(kwg_dyn);
  float* Nj = reinterpret_cast<float*>(kwg_dyn + KWG_UNION);
  float* Ls = Nj + BN;                         // [tpad][128]
  float* Rs = Ls + a.tpad * BN;                // [tpad][128]
  __shared__ double red[4][NRED];

  float negone;   // -1.0f the optimiser cannot see through (kv_wide.hpp)
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(negone));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int unit = blockIdx.x, db = blockIdx.y;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;
  const int jend = min(a.m, jbeg + a.jchunk);
  const int i = rb * 128 + wave * 32 + l31;
  const int nc = a.nc, nk = a.tpad >> 1;
  const float sc = a.wscale[0];
  const float ninorm = a.N1[min(i, a.n - 1)];

  for (int idx = tid; idx < a.tpad * BN; idx += NT) {
    const int c = idx >> 7, r = rb * 128 + (idx & 127);
    Ls[idx] = (c < a.tp && r < a.n) ? a.Lt[(int64_t)c * a.ldl + r] : 0.f;
  }

  u32x4 pz[4];
  auto load_z = [&](int j0, int c) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const _Float16* src = k == 0 ? a.Z1 + ((int64_t)rb * nc + c) * KW_TCH : a.Z2 + ((int64_t)(j0 / KW_TILE) * nc + c) * KW_TCH;
#pragma unroll
      for (int e = 0; e < 2; ++e) pz[2 * k + e] = *reinterpret_cast<const u32x4*>(src + (tid + NT * e) * 8);
    }
  };
  auto store_z = [&](int buf) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) *reinterpret_cast<u32x4*>(&Zs[buf * ZB + k * KW_TCH + (tid + NT * e) * 8]) = pz[2 * k + e];
  };
  // plane pair ss (0: z, 1: z^2 of dimensions 0..31 of the block; 2, 3: of dimensions 32..63) of the tile starting at j0
  auto load_t = [&](int j0, int ss) {
    const _Float16* src = a.T2 + ((((int64_t)(j0 / KW_TILE) * gridDim.y + db) * 4 + ss) * KWG_TBLK);
#pragma unroll
    for (int e = 0; e < 4; ++e) pz[e] = *reinterpret_cast<const u32x4*>(src + (tid + NT * e) * 8);
  };
  auto store_t = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = tid + NT * e;   // plane p >> 9, dimension (p >> 4) & 31, 8 positions from 8 (p & 15)
      *reinterpret_cast<u32x4*>(&Zs[buf * KWG_TBUF + ((p >> 9) * 32 + ((p >> 4) & 31)) * LDH + (p & 15) * 8]) = pz[e];
    }
  };

  const int boff = (h * KW_TILE + wave * 32 + l31) * 8;
  const int aoff = KW_TCH + (h * KW_TILE + l31) * 8;
  constexpr int LO = 2 * KW_TILE * 8;

  f32x16 acc[MODE ? 4 : 1];   // MODE 1: u, v of dimensions 0..31, u, v of dimensions 32..63 of the block
#pragma unroll
  for (int k = 0; k < (MODE ? 4 : 1); ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
  double d0 = 0.0, d1 = 0.0;   // sum W k;  MODE 0: sum A S, MODE 1: sc rs_i (this lane's half of the j rows)

  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    for (int idx = tid; idx < a.tpad * BN; idx += NT) {
      const int c = idx >> 7, j = j0 + (idx & 127);
      Rs[idx] = (c < a.tp && j < a.m) ? a.Rt[(int64_t)c * a.ldr + j] : 0.f;
    }
    if (tid < BN / 4) *reinterpret_cast<f32x4*>(&Nj[4 * tid]) = *reinterpret_cast<const f32x4*>(a.N2 + j0 + 4 * tid);   // (N2 is padded to whole tiles)
    load_z(j0, 0);
    store_z(0);
    __syncthreads();

    f32x16 sacc[JB];
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[jb][r] = 0.f;
    int buf = 0;
#pragma unroll 1
    for (int c = 0; c < nc; ++c, buf ^= 1) {
      const bool more = c + 1 < nc;
      if (more) load_z(j0, c + 1);
      const _Float16* zb = Zs + buf * ZB;
      const f16x8 bh = *reinterpret_cast<const f16x8*>(zb + boff);
      const f16x8 bl = *reinterpret_cast<const f16x8*>(zb + boff + LO);
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(zb + aoff + jb * 32 * 8);
        const f16x8 al = *reinterpret_cast<const f16x8*>(zb + aoff + jb * 32 * 8 + LO);
        sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, sacc[jb], 0, 0, 0);
        sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, sacc[jb], 0, 0, 0);
        sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, sacc[jb], 0, 0, 0);
      }
      if (more) store_z(buf ^ 1);
      __syncthreads();   // chunk c + 1 is staged; every wave is done with this buffer (after the last chunk: with both)
    }
    mfma_result_fence(sacc);   // the dot products are read on the VALU next (common.hpp)
    if constexpr (MODE) {
      load_t(j0, 0);
      store_t(0);
    }

    u32x4 ahi[MODE ? JB : 1][2], alo[MODE ? JB : 1][2];   // MODE 1: the split A sc tile, B operands of the second contraction
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int jp = 0; jp < JB / NQ; ++jp) {
      f32x16 wacc[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) wacc[q][r] = 0.f;
      for (int ks = 0; ks < nk; ++ks) {
        const float lv = Ls[(2 * ks + h) * BN + wave * 32 + l31];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          wacc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(Rs[(2 * ks + h) * BN + (NQ * jp + q) * 32 + l31], lv, wacc[q], 0, 0, 0);
      }
      mfma_result_fence(wacc);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int jb = NQ * jp + q;
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) {
          f32x4 nj[2];
#pragma unroll
          for (int g = 0; g < 2; ++g) nj[g] = *reinterpret_cast<const f32x4*>(&Nj[jb * 32 + 16 * mf + 8 * g + 4 * h]);
          u32x4 kh, kl;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            float av[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const int r = 8 * mf + 2 * p + e;
              const float nn = nj[p >> 1][2 * (p & 1) + e] + ninorm;
              const float sq = __builtin_fmaxf(__builtin_fmaf(sacc[jb][r], -2.f, nn), 0.f);
              float k, dk;
              wide_cov_dcov<KIND>(sq, k, dk);
              const float w = wacc[q][r];
              const float aw = w * dk;
              p0 = __builtin_fmaf(w, k, p0);
              if constexpr (MODE) {
                av[e] = aw * sc;
                p1 += av[e];
              } else {
                p1 = __builtin_fmaf(aw, sq, p1);
              }
            }
            if constexpr (MODE) {
              // hi rounded toward zero, lo = A - hi (kv_wide.hpp)
              typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
              const uint32_t hiw = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(av[0], av[1]));
              const f16x2 hv = __builtin_bit_cast(f16x2, hiw);
              const float l0 = __builtin_fmaf((float)hv[0], negone, av[0]);
              const float l1 = __builtin_fmaf((float)hv[1], negone, av[1]);
              kh[p] = hiw;
              kl[p] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(l0, l1));
            }
          }
          if constexpr (MODE) {
            ahi[jb][mf] = kh;
            alo[jb][mf] = kl;
          }
        }
      }
    }
    d0 += (double)p0;
    d1 += (double)p1;

    if constexpr (MODE) {
      __syncthreads();   // plane pair 0 is staged
#pragma unroll
      for (int ss = 0; ss < 4; ++ss) {
        if (ss < 3) load_t(j0, ss + 1);
        const _Float16* tb = Zs + (ss & 1) * KWG_TBUF;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
          for (int mf = 0; mf < 2; ++mf) {
            const int o = l31 * LDH + jb * 32 + 16 * mf + 8 * h;
            const f16x8 th = *reinterpret_cast<const f16x8*>(tb + o);
            const f16x8 tl = *reinterpret_cast<const f16x8*>(tb + 32 * LDH + o);
            const f16x8 khv = __builtin_bit_cast(f16x8, ahi[jb][mf]);
            const f16x8 klv = __builtin_bit_cast(f16x8, alo[jb][mf]);
            acc[ss] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, khv, acc[ss], 0, 0, 0);
            acc[ss] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, klv, acc[ss], 0, 0, 0);
            acc[ss] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, khv, acc[ss], 0, 0, 0);
          }
        if (ss < 3) store_t((ss + 1) & 1);
        __syncthreads();   // the next pair is staged; every wave is done with this one (after the last: with the tile's R rows and norms)
      }
    } else {
      __syncthreads();   // every wave is done with the R rows and the norms of this tile
    }
  }

  const double g0 = wave_sum(d0);
  if constexpr (MODE == 0) {
    const double g1 = wave_sum(d1);
    if (lane == 0) {
      red[wave][0] = g0;
      red[wave][1] = g1;
    }
    __syncthreads();
    if (tid < 2) a.part[(int64_t)unit * a.pstride + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  } else {
    mfma_result_fence(acc);   // the accumulators of the last contraction MFMAs are read next
    const double rs = d1 + __shfl_xor(d1, 32, 64);   // both halves of the j rows
    if (lane == 0) red[wave][0] = g0;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        __builtin_amdgcn_sched_barrier(0);   // one row load and one reduction at a time: hoisted, the 32 loads spill
        const int ql = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, q = db * KWG_DB + ql;
        const double z = (i < a.n && q < a.dp) ? (double)a.X1[(int64_t)i * a.dp + q] : 0.0;
        double v = z * z * rs - 2.0 * z * (double)acc[2 * b][r] + (double)acc[2 * b + 1][r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (l31 == 0) red[wave][1 + ql] = v;
      }
    __syncthreads();
    if (tid < NRED && (tid > 0 || db == 0)) {
      const int slot = tid == 0 ? 0 : 1 + db * KWG_DB + tid - 1;
      a.part[(int64_t)unit * a.pstride + slot] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
    if (a.U && i < a.n) {
      float* urow = a.U + ((int64_t)s * a.n + i) * a.dq + db * KWG_DB;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4 v = {acc[2 * b][4 * r4], acc[2 * b][4 * r4 + 1], acc[2 * b][4 * r4 + 2], acc[2 * b][4 * r4 + 3]};
          *reinterpret_cast<f32x4*>(urow + b * 32 + 8 * r4 + 4 * h) = v;
        }
      if (db == 0 && h == 0) a.RS[(int64_t)s * a.n + i] = (float)rs;
    }
  }
}

// out[o], o < nout: sums over the `units` partial rows in their fixed order.  MODE 0: out[0], out[1] (the single-lengthscale sum), zero behind;
// MODE 1: out[0], out[1 + q] = (1 / sc) sum, q < d, zero behind
__global__ __launch_bounds__(256) void wide_grad_reduce_kernel(const double* __restrict__ part, int units, int pstride, int mode, int d,
                                                               const float* __restrict__ wscale, float* __restrict__ out, int nout) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nout) return;
  const int live = mode ? 1 + d : 2;
  double acc = 0.0;
  if (o < live)
    for (int u = 0; u < units; ++u) acc += part[(int64_t)u * pstride + o];
  if (mode && o > 0) acc *= (double)wscale[1];
  out[o] = (float)acc;
}

// Gz1[i][q] = 2 (1 / sc) sum over the slabs of (z_iq sc rs_i - sc u_iq) in float64, slabs in their fixed order
__global__ __launch_bounds__(256) void wide_gz_reduce_kernel(const float* __restrict__ U, const float* __restrict__ RS, int slabs, int n, int d, int dq,
                                                             const float* __restrict__ X1, int dp, const float* __restrict__ wscale,
                                                             float* __restrict__ Gz, int64_t ldg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * d) return;
  const int i = (int)(e / d), q = (int)(e - (int64_t)i * d);
  const double z = (double)X1[(int64_t)i * dp + q];
  double acc = 0.0;
  for (int sl = 0; sl < slabs; ++sl)
    acc += z * (double)RS[(int64_t)sl * n + i] - (double)U[((int64_t)sl * n + i) * dq + q];
  Gz[(int64_t)i * ldg + q] = (float)(2.0 * (double)wscale[1] * acc);
}

}  // namespace gpamd
