// Fused bilinear derivative for WIDE inputs, 33 .. 512 dimensions, by DIRECT DIFFERENCES (RBF, Matern 1/2, 3/2, 5/2): the derivative kernel of
// kv_wide_direct.hpp, for the clouds kv_wide_grad.hpp must refuse (max |z|^2 > 32, every Matern 1/2 cloud).
//
//   g[0] = sum_ij W_ij k_ij,   g[1 + q] = sum_ij A_ij (z_iq - z_jq)^2,   Gz1[i] = 2 sum_j A_ij (z_i - z_j),   W = L^T R,  A = W o dk/ds
//
// the contract of kv_grad2.hpp and kv_wide_grad.hpp (LinearOperator._bilinear_derivative on the kernel operator + the dense backward of
// gpytorch/functions/rbf_covariance.py:26-29, matern_covariance.py:53-56; input gradients as the KeOps precedent provides them); until now these clouds
// formed W as dense row blocks with a library GEMM (backend.kv_grad_generic) and had no input gradients at all.
//
// 256 threads, 4 waves; a workgroup owns 256 output rows (NI = 2: wave w owns rows 64 w .. + 63 as two 32-row tiles) and one j chunk of a split-j plan,
// the j tile is 128 rows.  Per j tile:
//   * FIRST SWEEP, the distances: kv_wide_direct_kernel's, unchanged -- the plain float32 prepared rows, z_j chunks of 16 dimensions transposed and
//     double-buffered in LDS (Xf[k][j], row stride 132 floats), one broadcast ds_read_b128 per dimension and quad, each lane's own z_i row from global
//     memory one chunk ahead, one packed subtraction and one packed multiply-add per pair of adjacent j.  Lane (i = l31, h) ends with S of the pairs
//     (j(r, h), i), j(r, h) = (r & 3) + 8 (r >> 2) + 4 h, of the 4 x NI 32 x 32 blocks: 128 registers.
//   * W tile (kv_wide_grad.hpp's): W_ij = sum_c L_ci R_cj on v_mfma_f32_32x32x2_f32, R as the A operand (rows j) and L as the B operand (rows i), so the
//     result lands in the slots of S.  L [t][256] is staged in LDS once per workgroup, R [t][128] once per j tile; per j block the two row tiles run
//     interleaved and share the R operand.  Plain f32 products, no split.  Up to KWDG_MAXT = 66 columns per pass; more run as further passes whose
//     sums add (g is linear in W), each regenerating S.
//   * k and dk/ds from S (wide_cov_dcov; Matern 1/2: k = e^-r, dk/ds = -e^-r / (2 r) from one v_rsq_f32, 0 where S = 0 -- the diagonal of a symmetric
//     product has S = 0 exactly), sum W k per lane in f32 within the tile and in float64 across tiles.
//     MODE 0 (one lengthscale, no input gradients): sum A S likewise, and the tile is done: the forward's distance sweep + the W tile + ~10 VALU
//     instructions per pair.
//   * MODE 1 (per-dimension sums, optionally Gz1), SECOND SWEEP over the chunks of the same j tile with A in the registers that held S.  The sums are formed
//     from the differences themselves -- NOT from z_i^2 rs_i - 2 z_i u_i + v_i as kv_wide_grad.hpp does: that cancels in proportion to |z|^2, and these
//     are the clouds where |z|^2 is large.  Per dimension, quad and pair of adjacent j:  df = z_i - z_j,  t = A df,  gz += t,  gq = fma(t, df, gq)
//     -- four packed instructions against the first sweep's two.  The loop order is turned round: DIMENSION outer, quads inner, 4 dimensions at a time,
//     so a lane carries 4 x (NI + 1) packed accumulators (24 registers) and not 16 per quantity and chunk; the z_j chunk in LDS serves all of it, the
//     lane's z_i come 4 dimensions at a time from global memory, one group ahead.  Behind every group of 4 dimensions:
//       - Gz1 needs no sum across rows: the two half-waves exchange one row tile each (4 lane exchanges), and lane (i, h) adds the 4 values of row tile
//         ni = h to ITS row of the per-slab workspace G [S][n][dq] with one 16-byte load and store.  The workgroup owns (slab, row block), the first j
//         tile stores and later tiles add: no clear pass, no atomics.  wide_direct_gz_reduce_kernel sums the slabs in float64.
//       - g_q: the 4 per-lane values are summed over the 64 lanes by a halving butterfly (2 + 1 + 4 = 7 lane exchanges: the halves keep two dimensions
//         each, the quarters one) and added in float64 to the wave's own row of an LDS table [4][dq]; the workgroup writes float64 partials [unit][1 + dq],
//         wide_direct_grad_reduce_kernel sums the units in their fixed order.
// Budget per wave and 16-dimension chunk.  First sweep: 256 ds_read_b128, 2048 packed VALU (kv_wide_direct.hpp).  Second sweep: the same 256
// ds_read_b128 (NI = 2 row tiles share every quad: 8 cycles of the CU's LDS pipe x 4 waves = 32 against 16 packed instructions = 64 SIMD cycles per
// read -- VALU-bound; NI = 1 would be 32 against 32 with half the rows per read), 4096 packed VALU, and per 4 dimensions 4 + 7 lane exchanges, 14
// selects, one 16-byte global read-modify-write and one f64 LDS add: < 3 % on top.  Half-chunks or dimension blocks on a grid axis would regenerate
// S and W per block (kv_wide_grad.hpp pays that: eight times the Gram work at d = 512); here S and W are formed once per j tile whatever d.
// LDS (dynamic): g_q table 32 dq B (MODE 1) + z_j buffers 16.5 KB + L and R tiles 1.5 KB per column -- 11 columns: 38 KB, 65 columns: 132 KB at d = 512,
// one workgroup per CU.
// No atomics, a fixed summation order: two calls give the same bits.  Rows beyond n / m: the staged L / R tiles are zero there, so W = 0 against
// finite k (rows j beyond jend and dimensions beyond dp are staged as zeros, a row i beyond n repeats the last one and is never written).
// Sizing (from -Rpass-analysis=kernel-resource-usage over the eight instantiations; the Makefile fails the build on scratch): see the figures in front
// of KWDG_NI.
#pragma once
#include "kv_wide_direct.hpp"
#include "kv_wide_grad.hpp"

namespace gpamd {

// First sweep: 128 registers of S, 32 + 32 of z_i (this chunk, the next), 64 of z_j quads (two groups of 8 reads), 8 of z_j staging -- more than 256, as
// in the forward: the allocator parks the surplus in AGPRs (v_accvgpr moves, ~50 per chunk against 2048 packed instructions).  Second sweep: 128 of A, 24
// packed accumulators, 8 + 8 of z_i groups, 32 of z_j quads, 8 of z_j staging: 4 AGPR moves per 1024 packed instructions.  The W stage keeps its 32
// accumulators in AGPRs.  From the build's remarks, all four kinds alike: MODE 0 256 VGPRs + 84 AGPRs, MODE 1 256 VGPRs + 52 .. 56 AGPRs, no scratch,
// one wave per SIMD (LDS admits one workgroup per CU beyond 40 columns anyway).  Three places are pinned with volatile asms because the optimiser
// otherwise moves code to where registers are taken (5 KB of scratch per lane): the arithmetic of a second-sweep group (it sank behind all 64 reads of
// the 4 dimensions), the covariance stage of a j block (it sank behind the four W tiles), and the addresses of the W stage (hoisted out of the tile loop).
constexpr int KWDG_NI = 2;
constexpr int KWDG_BM = 4 * 32 * KWDG_NI;       // output rows per workgroup
constexpr int KWDG_MAXT = 66;                   // columns per pass
constexpr int kwdg_dq(int d) { return KW_CHUNK * kw_chunks(d); }
constexpr size_t kwdg_lds(int tpad, int dq, int mode) {
  return (mode ? (size_t)4 * dq * sizeof(double) : 0) + (size_t)2 * KWD_XB * sizeof(float) + (size_t)tpad * (KWDG_BM + KW_TILE) * sizeof(float);
}

struct KvWideDirectGradArgs {
  const float* X1;        // [n][dp], [m][dp]: the prepared rows
  const float* X2;
  const float* Lt;        // [tp][ldl], [tp][ldr]: the columns of this pass
  const float* Rt;
  int64_t ldl, ldr;
  int n, m, dp, nc, tp, tpad;
  int S, jchunk, nrb;
  double* part;           // [nrb S][pstride]: MODE 0 (sum W k, sum A S); MODE 1 (sum W k | per-dimension sums [dq])
  int pstride;
  float* G;               // optional [S][n][dq]: sum_j A_ij (z_i - z_j) of this slab (input gradients) or nullptr
  int dq;                 // 16 chunks
  int add;                // a later pass: the first j tile adds to G as well
};

template <int KIND>
__device__ __forceinline__ void wide_direct_cov_dcov(float s, float& k, float& dk) {
  if constexpr (KIND == KIND_MATERN12) {
    const float ri = s > 0.f ? __builtin_amdgcn_rsqf(s) : 0.f;   // (S = 0: r = 0, k = 1, dk/ds := 0)
    const float e = __builtin_amdgcn_exp2f(-(s * ri) * 1.4426950408889634f);
    k = e;
    dk = -0.5f * e * ri;
  } else {
    wide_cov_dcov<KIND>(s, k, dk);
  }
}

template <int KIND, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void kv_wide_direct_grad_kernel(KvWideDirectGradArgs a) {
  static_assert(KIND == KIND_RBF || KIND == KIND_MATERN12 || KIND == KIND_MATERN32 || KIND == KIND_MATERN52, "RBF, Matern 1/2, 3/2, 5/2");
  static_assert(MODE == 0 || MODE == 1, "one lengthscale, or per dimension (Gz1: a.G)");
  constexpr int NI = KWDG_NI, NT = 256, BN = KW_TILE, BM = KWDG_BM, JB = BN / 32;
  constexpr int LDJ = KWD_LDJ, XB = KWD_XB, KC = KW_CHUNK;
  static_assert(NT == 2 * BN && NI == 2, "two threads stage one row of the j tile; the half-waves share the two row tiles of Gz1");
  extern __shared__ __attribute__((aligned(16))) unsigned char kwdg_dyn[];
  double* Gq = reinterpret_cast<double*>(kwdg_dyn);                                                  // [4][dq] (MODE 1)
  float* Xf = reinterpret_cast<float*>(kwdg_dyn + (MODE ? (size_t)4 * a.dq * sizeof(double) : 0));   // [buf][k][j]
  float* Ls = Xf + 2 * XB;                                                                           // [tpad][256]
  float* Rs = Ls + a.tpad * BM;                                                                      // [tpad][128]
  __shared__ double red[4][2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;                  // multiple of BN
  const int jend = min(a.m, jbeg + a.jchunk);
  const int ibase = rb * BM + wave * (NI * 32);
  const int nc = a.nc, dp = a.dp, nk = a.tpad >> 1, dq = a.dq;

  for (int idx = tid; idx < a.tpad * BM; idx += NT) {
    const int c = idx / BM, r = rb * BM + (idx % BM);
    Ls[idx] = (c < a.tp && r < a.n) ? a.Lt[(int64_t)c * a.ldl + r] : 0.f;
  }
  if constexpr (MODE) {
    for (int q = lane; q < dq; q += 64) Gq[wave * dq + q] = 0.0;   // the wave's own row: no barrier between it and the wave's adds
  }

  // chunk c of this lane's own rows (a row beyond n repeats the last one: never written) and of the j tile starting at j0: global -> registers
  const float* xi[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) xi[ni] = a.X1 + (int64_t)min(ibase + ni * 32 + l31, a.n - 1) * dp;
  const int jr = tid >> 1, hh = tid & 1;
  f32x4 zin[NI][KC / 4], pj[2];
  auto load_zi = [&](int c) {
    const int k0 = KC * c;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int g = 0; g < KC / 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k0 + 4 * g < dp) v = *reinterpret_cast<const f32x4*>(xi[ni] + k0 + 4 * g);
        zin[ni][g] = v;
      }
  };
  auto load_zj = [&](int j0, int c) {
    const int k0 = KC * c, j = j0 + jr;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};   // rows beyond jend, dimensions beyond dp: zero (k stays finite against W = 0)
      if (j < jend && k0 + 8 * hh + 4 * g < dp) v = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * dp + k0 + 8 * hh + 4 * g);
      pj[g] = v;
    }
  };
  auto store_zj = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 8; ++e) Xf[buf * XB + (8 * hh + e) * LDJ + jr] = pj[e >> 2][e & 3];
  };

  load_zj(jbeg, 0);
  if constexpr (MODE == 0) load_zi(0);
  store_zj(0);
  __syncthreads();   // (the L tile too)

  double d0 = 0.0, d1 = 0.0;   // sum W k;  MODE 0: sum A S
  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    if constexpr (MODE) load_zi(0);   // (the second sweep has its own z_i stream: nothing of the next tile is loaded ahead across it)
    // ---- first sweep (kv_wide_direct.hpp): S of the pairs (j(r, h) of block jb, i): sq[ni][jb][r]
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
      if constexpr (MODE) {   // behind the last chunk: chunk 0 of the SAME tile again, for the second sweep
        if (!last) load_zi(c + 1);
        load_zj(j0, last ? 0 : c + 1);
      } else {                // behind the last chunk of the last tile: the lane's chunk 0 again and an all-zero tile, never used
        load_zi(last ? 0 : c + 1);
        load_zj(last ? j0 + BN : j0, last ? 0 : c + 1);
      }
      const float* xb = Xf + buf * XB + 4 * h;
      constexpr int KG = 8, NG = 4 * JB * (KC / KG);
      f32x4 zq[2][KG];
      auto read_group = [&](int u, f32x4* dst) {
        const int g = u / (KC / KG), kh = u % (KC / KG);
#pragma unroll
        for (int k = 0; k < KG; ++k) dst[k] = *reinterpret_cast<const f32x4*>(xb + (KG * kh + k) * LDJ + 8 * g);
      };
      read_group(0, zq[0]);
#pragma unroll
      for (int u = 0; u < NG; ++u) {
        if (u + 1 < NG) read_group(u + 1, zq[(u + 1) & 1]);
        asm volatile("" ::: "memory");   // no read of a later group moves up past here
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
      store_zj(buf ^ 1);   // unconditional, as in the forward
      __syncthreads();     // the next chunk is staged; every wave is done with this buffer
    }

    // ---- R tile (the W stage of the previous tile lies behind the barriers of this tile's sweep), W tile, covariance
    // (the thread index through an asm: the addresses of this stage are formed here, per tile -- hoisted out of the tile loop they would be carried
    // across both sweeps, where every register is taken, and spilled)
    int tv = tid;
    asm volatile("" : "+v"(tv));
    for (int idx = tv; idx < a.tpad * BN; idx += NT) {
      const int c = idx / BN, j = j0 + (idx % BN);
      Rs[idx] = (c < a.tp && j < a.m) ? a.Rt[(int64_t)c * a.ldr + j] : 0.f;
    }
    __syncthreads();
    const float* rsp = Rs + ((tv >> 5) & 1) * BN + (tv & 31);                          // row h of a column pair, position l31 of a j block
    const float* lsp = Ls + ((tv >> 5) & 1) * BM + (tv >> 6) * (NI * 32) + (tv & 31);   // ... of the wave's first row tile
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      f32x16 wacc[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) wacc[ni][r] = 0.f;
      for (int ks = 0; ks < nk; ++ks) {
        const float rv = rsp[2 * ks * BN + jb * 32];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) wacc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(rv, lsp[2 * ks * BM + ni * 32], wacc[ni], 0, 0, 0);
      }
      mfma_result_fence(wacc);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float sv = sq[ni][jb][r];
          float k, dk;
          wide_direct_cov_dcov<KIND>(sv, k, dk);
          const float w = wacc[ni][r];
          const float aw = w * dk;
          p0 = __builtin_fmaf(w, k, p0);
          if constexpr (MODE) {
            sq[ni][jb][r] = aw;
          } else {
            p1 = __builtin_fmaf(aw, sv, p1);
          }
        }
      // the block's covariance stage stays in front of the next block's MFMAs: A is read only in the second sweep, and the optimiser would sink the
      // four stages there, with the 128 W values live beside the 128 of S
      if constexpr (MODE) asm volatile("" : "+v"(sq[0][jb]), "+v"(sq[1][jb]), "+v"(p0));
    }
    d0 += (double)p0;
    d1 += (double)p1;

    // ---- second sweep: per-dimension sums and Gz1 from the differences, A in sq
    if constexpr (MODE) {
      const bool first = j0 == jbeg && !a.add;
      const int irow = ibase + h * 32 + l31;   // the row whose Gz1 values this lane writes (row tile ni = h)
      float* grow = a.G ? a.G + ((int64_t)s * a.n + min(irow, a.n - 1)) * dq : nullptr;
      f32x4 zn[NI];   // the lane's z_i, 4 dimensions at a time, one group ahead
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) zn[ni] = *reinterpret_cast<const f32x4*>(xi[ni]);
#pragma unroll 1
      for (int c = 0; c < nc; ++c, buf ^= 1) {
        const bool last = c == nc - 1;
        load_zj(last ? j0 + BN : j0, last ? 0 : c + 1);   // (behind the last tile: an all-zero tile, never used)
#pragma unroll 1
        for (int g4 = 0; g4 < KC / 4; ++g4) {
          const int k0 = KC * c + 4 * g4;
          f32x4 zc[NI];
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            zc[ni] = zn[ni];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};   // dimensions beyond dp: zero, as the staged z_j (dp % 4 == 0)
            if (k0 + 4 < dp) v = *reinterpret_cast<const f32x4*>(xi[ni] + k0 + 4);
            zn[ni] = v;
          }
          f32x4 gold = {0.f, 0.f, 0.f, 0.f};
          if (grow && !first && irow < a.n) gold = *reinterpret_cast<const f32x4*>(grow + k0);
          const float* xk = Xf + buf * XB + 4 * h + 4 * g4 * LDJ;
          f32x2 gz2[NI][4], gq2[4];
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            gq2[kk] = (f32x2)(0.f);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) gz2[ni][kk] = (f32x2)(0.f);
          }
          // A group = dimension kk of the four, the 4 quads of j block jb: 4 reads, 64 packed instructions; reads one group ahead, pinned as above
          constexpr int NG2 = 4 * JB;
          f32x4 zq[2][4];
          auto read_group = [&](int v, f32x4* dst) {
            const int kk = v / JB, jb = v % JB;
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = *reinterpret_cast<const f32x4*>(xk + kk * LDJ + 32 * jb + 8 * q);
          };
          read_group(0, zq[0]);
#pragma unroll
          for (int v = 0; v < NG2; ++v) {
            if (v + 1 < NG2) read_group(v + 1, zq[(v + 1) & 1]);
            asm volatile("" ::: "memory");
            const int kk = v / JB, jb = v % JB;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int ni = 0; ni < NI; ++ni) {
                const f32x2 z = (f32x2)(zc[ni][kk]);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                  const f32x2 df = z - (f32x2){zq[v & 1][q][2 * p], zq[v & 1][q][2 * p + 1]};
                  const f32x2 t = (f32x2){sq[ni][jb][4 * q + 2 * p], sq[ni][jb][4 * q + 2 * p + 1]} * df;
                  gz2[ni][kk] += t;
                  gq2[kk] = __builtin_elementwise_fma(t, df, gq2[kk]);
                }
              }
            // the group's arithmetic stays in the group: its results are read only behind the branches below, where the optimiser would sink all of it
            // to, away from its reads (volatile asms keep their order among themselves)
            asm volatile("" : "+v"(gq2[kk]), "+v"(gz2[0][kk]), "+v"(gz2[1][kk]));
            __builtin_amdgcn_sched_barrier(0);
          }
          // Gz1: the half-waves exchange one row tile each; lane (i, h) owns row tile ni = h
          if (grow) {
            f32x4 mine;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const float g0 = gz2[0][kk][0] + gz2[0][kk][1], g1 = gz2[1][kk][0] + gz2[1][kk][1];
              const float keep = h ? g1 : g0, send = h ? g0 : g1;
              mine[kk] = keep + __shfl_xor(send, 32, 64);
            }
            if (irow < a.n) *reinterpret_cast<f32x4*>(grow + k0) = gold + mine;
          }
          // g_q: halving butterfly over the 64 lanes -- half h keeps dimensions 2 h, 2 h + 1, quarter b of it dimension 2 h + b
          {
            float gq[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) gq[kk] = gq2[kk][0] + gq2[kk][1];
            float ka = h ? gq[2] : gq[0], kb = h ? gq[3] : gq[1];
            ka += __shfl_xor(h ? gq[0] : gq[2], 32, 64);
            kb += __shfl_xor(h ? gq[1] : gq[3], 32, 64);
            const int b = (lane >> 4) & 1;
            float kp = b ? kb : ka;
            kp += __shfl_xor(b ? ka : kb, 16, 64);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) kp += __shfl_xor(kp, o, 64);
            if ((lane & 15) == 0) Gq[wave * dq + k0 + 2 * h + b] += (double)kp;
          }
        }
        store_zj(buf ^ 1);
        __syncthreads();   // the next chunk is staged; every wave is done with this buffer (behind the last: with the R tile as well)
      }
    }
  }

  const double g0 = wave_sum(d0);
  const double g1 = wave_sum(d1);
  int te = threadIdx.x;   // (as above: nothing of the epilogue is carried through the loops)
  asm volatile("" : "+v"(te));
  if ((te & 63) == 0) {
    red[te >> 6][0] = g0;
    red[te >> 6][1] = g1;
  }
  __syncthreads();
  double* prow = a.part + (int64_t)unit * a.pstride;
  if (te < (MODE ? 1 : 2)) prow[te] = ((red[0][te] + red[1][te]) + red[2][te]) + red[3][te];
  if constexpr (MODE) {
    for (int q = te; q < dq; q += NT) prow[1 + q] = ((Gq[q] + Gq[dq + q]) + Gq[2 * dq + q]) + Gq[3 * dq + q];
  }
}

// out[o], o < nout: sums over the `units` partial rows in their fixed order.  mode 0: out[0], out[1] (the single-lengthscale sum), zero behind;
// else out[0], out[1 + q], q < d, zero behind
__global__ __launch_bounds__(256) void wide_direct_grad_reduce_kernel(const double* __restrict__ part, int units, int pstride, int mode, int d,
                                                                      float* __restrict__ out, int nout) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nout) return;
  const int live = mode ? 1 + d : 2;
  double acc = 0.0;
  if (o < live)
    for (int u = 0; u < units; ++u) acc += part[(int64_t)u * pstride + o];
  out[o] = (float)acc;
}

// Gz1[i][q] = 2 sum over the slabs of G[slab][i][q] in float64, slabs in their fixed order
__global__ __launch_bounds__(256) void wide_direct_gz_reduce_kernel(const float* __restrict__ G, int slabs, int n, int d, int dq, float* __restrict__ Gz,
                                                                    int64_t ldg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * d) return;
  const int i = (int)(e / d), q = (int)(e - (int64_t)i * d);
  double acc = 0.0;
  for (int sl = 0; sl < slabs; ++sl) acc += (double)G[((int64_t)sl * n + i) * dq + q];
  Gz[(int64_t)i * ldg + q] = (float)(2.0 * acc);
}

}  // namespace gpamd
