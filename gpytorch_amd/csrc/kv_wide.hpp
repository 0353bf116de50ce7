// Fused covariance MVM for WIDE inputs, 33 .. 512 dimensions (RBF, Matern 3/2, 5/2): the number of dimensions is a RUN-TIME reduction loop, not a
// template parameter.  The kernels of kv_gramh.hpp hold the split x_i of a row in registers, one instantiation per D; beyond 32 dimensions that
// cannot go on (at D > 20 they already run one wave per SIMD).  Here the shape is flash attention's: for every 128-row j tile the products
// z_j . z_i accumulate over 16-dimension chunks in f32 MFMA accumulators, the covariance is applied element by element, and K contracts with V --
// all three on v_mfma_f32_32x32x16_f16 at f32 accuracy, as in kv_gramh.hpp.  The reference has no dimension limit (gpytorch/kernels/kernel.py:26-49
// forms the distances with one matmul of any width); until now such clouds went through dense row blocks of K and a library GEMM (backend.kv_chunked).
//
// Split image of a cloud (wide_split_kernel, once per prepared cloud).  Prepared rows float[n][dp] become two f16 planes hi = f16(z),
// lo = f16(z - hi) (f16_split, gram_f16.hpp) in the order the MFMA operand reads them: per 128-row tile, per chunk, per plane, per k-half h,
// [row][8 x f16] -- a tile-chunk is 8 KB of contiguous memory, staging it is a 16-byte-per-thread copy, and lane (row, h) reads its operand with one
// ds_read_b128, consecutive rows 16 bytes apart (the conflict-free layout of gram_a_off).  Rows beyond n and dimensions beyond d are zero.  The A
// operand (contracted rows z_j) and the B operand (output rows z_i) of the 32x32x16 MFMA take k-slots 8 h .. 8 h + 7 from the same positions, so ONE
// image serves both roles and k(x, x) needs one image.
//
// The norms travel as f32 beside the image (wide_norm_kernel) and are added on the VALU:  S = max(|z_i|^2 + |z_j|^2 - 2 dot, 0), one packed add and
// one packed multiply-add per two elements.  Not through one more MFMA with norm slots (gram_pack_*), for two reasons: that form needs [n_h, n_l, 1, 1]
// on the contracted side and [1, 1, n_h, n_l] on the output side, i.e. two images per cloud; and a split f16 norm carries 22 bits where the f32 norm
// carries 24 -- at the selection limit |z|^2 = 32 that is the larger part of the cancellation error.  The norm is that of the STORED operand,
// sum_k (hi_k + lo_k)^2 accumulated in float64: what remains is the rounding of the coordinates themselves (2^-22 relative, an error in S that scales
// with |z_i - z_j|, not with |z|^2), the dropped lo * lo term (<= 2^-22 |z_i| |z_j|, as GramF16 drops it for D >= 12) and the f32 accumulation.
//
// Main kernel.  256 threads, 4 waves; a workgroup owns 128 NI output rows (wave w: rows 32 NI w ..) and one j chunk of the split-j plan; slabs, the
// done flag, the V planes (KvhArgs, vsplit_kernel), colmul and the epilogue are kv_gramh.hpp's.  Per j tile:
//   * a run-time loop over the d-chunks: the z_i chunks of the row block (NI tile-chunks) and the z_j chunk of the tile sit in LDS, DOUBLE-BUFFERED --
//     the global loads of chunk c + 1 (of chunk 0 of the next tile after the last) are issued before the MFMAs of chunk c and stored behind them, one
//     barrier per chunk.  A wave reads its NI B operands (hi, lo) once per chunk and one A pair per 32-row j block: 8 + 2 NI ds_read_b128 for 12 NI MFMAs
//     (hi.hi, hi.lo, lo.hi per 32 x 32 block) into 4 NI accumulators of 16 registers.  At NI = 1 the LDS reads take about as long as the MFMAs they
//     feed (4 waves x 10 reads x 8 cycles against 12 x 32 cycles per SIMD); NI = 2 halves that;
//   * mfma_result_fence over the 4 NI accumulators, then per (j block, row tile): S, K = 2^KSHIFT k(S) (cov_pair_from_sq, the packed form of cov_scaled),
//     its hi/lo split as kv_gramh_body.inc forms it (v_cvt_pkrtz, v_fma_mix with the opaque -1), three MFMAs per 16 contracted rows and column tile, the
//     extra column on the VALU.  The V planes, the norms and the extra column of the NEXT tile are loaded into registers before the contraction and
//     stored behind the barrier that ends it.
// The schedule is that and no more: the generation of tile T is not overlapped with the Gram MFMAs of tile T + 1.
// Sizing (from -Rpass-analysis=kernel-resource-usage; the Makefile fails the build on scratch).  The library instantiates NI = 1: 64 + 16 CT
// accumulator registers, 16 staging registers, 16 CT for the next V planes -- 167 .. 242 VGPRs over the twelve instantiations, no scratch, two waves
// per SIMD; LDS 32 KB of z chunks + 17.4 CT KB of V planes + 1 KB: 50 KB (CT = 1), 67 KB (CT = 2), two workgroups per CU within the 160 KB, which is
// what covers a workgroup's barriers.  NI = 2 (128 + 32 CT accumulators, one wave per SIMD, 84 KB) halves the LDS operand traffic per MFMA, but the
// allocator left 12 - 16 bytes of scratch per lane in seven of its twelve instantiations with all 512 registers in use: not instantiated.
// Columns.  Every t from 1 to 65 runs on this one family (CT = 1, 2 column tiles of 32, EX = the 33rd / 65th column on the VALU): from d = 64 on the
// Gram MFMAs (3 per chunk and 32 x 32 block: 12 at d = 64) outweigh the contraction (6 CT), so a few-column variant would save little.  More
// columns run in launch groups of 64 (+ 1), and EVERY GROUP REGENERATES K: t = 128 costs twice the Gram work of t = 64.
#pragma once
#include "kv_gramh.hpp"

namespace gpamd {

constexpr int KW_MIN_DIM = 33, KW_MAX_DIM = 512;
constexpr int KW_CHUNK = 16;                 // dimensions per chunk: the k extent of one v_mfma_f32_32x32x16_f16
constexpr int KW_TILE = 128;                 // rows per image tile = the j tile
constexpr int KW_TCH = 4 * KW_TILE * 8;      // f16 elements of one tile-chunk: [plane][h][row][8]
constexpr int kw_chunks(int d) { return (d + KW_CHUNK - 1) / KW_CHUNK; }
constexpr int kw_tiles(int n) { return (n + KW_TILE - 1) / KW_TILE; }
constexpr int KW_NI = 1;                     // 32-row tiles per wave of the instantiated kernels (Sizing, above): 128 rows per workgroup
constexpr int kw_waves(int ni) { return ni == 1 ? 2 : 1; }   // resident waves per SIMD the register allocator is held to

struct KvWideArgs {
  KvhArgs h;              // a.X1, a.X2 unused (the images below); Vt: only the extra column is read from it
  const _Float16* Z1;     // split image of the output rows: [tiles][chunks][KW_TCH]
  const _Float16* Z2;     // ... of the contracted rows
  const float* N1;        // |z|^2 of the stored operands, [128 tiles], zero beyond the cloud
  const float* N2;
  int nc;                 // chunks
};

// ---- pre-pass.  Grid (tiles, chunks), 256 threads = 128 rows x 2 k-halves: thread (row, h) splits dimensions 16 c + 8 h .. + 7 of its row
__global__ __launch_bounds__(256) void wide_split_kernel(const float* __restrict__ Xp, int n, int dp, _Float16* __restrict__ Z, int nc) {
  const int tile = blockIdx.x, c = blockIdx.y;
  const int row = threadIdx.x >> 1, h = threadIdx.x & 1;
  const int i = tile * KW_TILE + row, k0 = KW_CHUNK * c + 8 * h;
  f16x8 hi, lo;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < n && k0 + 4 * g < dp) v = *reinterpret_cast<const f32x4*>(Xp + (int64_t)i * dp + k0 + 4 * g);   // (dp % 4 == 0; zeros beyond d: prep_points)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      _Float16 a, b;
      f16_split(v[e], a, b);
      hi[4 * g + e] = a;
      lo[4 * g + e] = b;
    }
  }
  _Float16* dst = Z + ((int64_t)tile * nc + c) * KW_TCH + (h * KW_TILE + row) * 8;
  *reinterpret_cast<f16x8*>(dst) = hi;
  *reinterpret_cast<f16x8*>(dst + 2 * KW_TILE * 8) = lo;
}

// One wave per row: N[i] = sum_k (hi_k + lo_k)^2 in float64 (the norm of what wide_split_kernel stored), zero for the rows that pad the last tile
__global__ __launch_bounds__(256) void wide_norm_kernel(const float* __restrict__ Xp, int n, int dp, float* __restrict__ N, int npad) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= npad) return;
  double acc = 0.0;
  if (i < n) {
    for (int k = 4 * lane; k < dp; k += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(Xp + (int64_t)i * dp + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        _Float16 a, b;
        f16_split(v[e], a, b);
        const double s = (double)(float)a + (double)(float)b;
        acc += s * s;
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) N[i] = (float)acc;
}

// the column maxima of the V pre-pass start from zero (a kernel, not a memset node: the launches may be captured)
__global__ void wide_clear_kernel(unsigned* p, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = 0u;
}

template <int KIND, int CT, int NI, int EX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kw_waves(NI), kw_waves(NI))))
void kv_wide_kernel(KvWideArgs wa) {
  static_assert(KIND == KIND_RBF || KIND == KIND_MATERN32 || KIND == KIND_MATERN52, "RBF, Matern 3/2, 5/2 (Matern 1/2 has a cusp at S = 0)");
  static_assert((CT == 1 || CT == 2) && (NI == 1 || NI == 2), "one or two column tiles, one or two row tiles per wave");
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int BN = KGH_BN, LDH = KGH_LDH, TC = 32 * CT, JB = BN / 32;
  constexpr int ZB = (NI + 1) * KW_TCH;        // f16 elements of one staging buffer: NI z_i tile-chunks, then the z_j tile-chunk
  constexpr int ZQ = 2 * (NI + 1);             // 16-byte pieces per thread and buffer
  constexpr int VQ = TC * (BN / 8) / NT;       // 16-byte pieces per thread and V plane
  static_assert(BN == KW_TILE, "the j tile is one image tile");
  const KvhArgs& ka = wa.h;
  const KvArgs& a = ka.a;
  __shared__ __attribute__((aligned(16))) _Float16 Vhs[TC * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 Vls[TC * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 Zs[2 * ZB];
  __shared__ __attribute__((aligned(16))) float Nj[BN];
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
  const int nc = wa.nc;
  const int last_tile = kw_tiles(a.n) - 1;        // a ragged last row block stages its last tile twice (rows beyond n are never written)

  float ninorm[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) ninorm[ni] = wa.N1[min(ibase + ni * 32 + l31, a.n - 1)];

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

  // chunk c of the row block and of the j tile starting at j0: global -> registers, registers -> buffer `buf`
  u32x4 pz[ZQ];
  auto load_z = [&](int j0, int c) {
#pragma unroll
    for (int k = 0; k <= NI; ++k) {
      const _Float16* src = k < NI ? wa.Z1 + ((int64_t)min(rb * NI + k, last_tile) * nc + c) * KW_TCH : wa.Z2 + ((int64_t)(j0 / KW_TILE) * nc + c) * KW_TCH;
#pragma unroll
      for (int e = 0; e < 2; ++e) pz[2 * k + e] = *reinterpret_cast<const u32x4*>(src + (tid + NT * e) * 8);
    }
  };
  auto store_z = [&](int buf) {
#pragma unroll
    for (int k = 0; k <= NI; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) *reinterpret_cast<u32x4*>(&Zs[buf * ZB + k * KW_TCH + (tid + NT * e) * 8]) = pz[2 * k + e];
  };
  // V planes, norms and extra column of the tile starting at j0 (rows beyond jend: zero planes, zero extra column; the image rows there are zero too, so
  // K stays finite against V = 0)
  u32x4 pvh[VQ], pvl[VQ];
  f32x4 pn = {0.f, 0.f, 0.f, 0.f}, pe = {0.f, 0.f, 0.f, 0.f};
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
    if (tid < BN / 4) pn = *reinterpret_cast<const f32x4*>(wa.N2 + j0 + 4 * tid);   // (N2 is padded to whole tiles)
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
    if (tid < BN / 4) *reinterpret_cast<f32x4*>(&Nj[4 * tid]) = pn;
    if constexpr (EX) {
      if (tid >= BN && tid < BN + BN / 4) *reinterpret_cast<f32x4*>(&Es[4 * (tid - BN)]) = pe;
    }
  };

  // this wave's B operands sit in tile-chunk (row in block) / 128 of the buffer, at row (row in block) % 128
  int boff[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int r = wave * (NI * 32) + ni * 32 + l31;
    boff[ni] = (r / KW_TILE) * KW_TCH + (h * KW_TILE + (r % KW_TILE)) * 8;
  }
  const int aoff = NI * KW_TCH + (h * KW_TILE + l31) * 8;
  constexpr int LO = 2 * KW_TILE * 8;   // the lo plane of a tile-chunk

  load_z(jbeg, 0);
  load_v(jbeg);
  store_z(0);
  store_v();
  __syncthreads();

  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    const bool more_tiles = j0 + BN < jend;
    f32x16 sacc[NI][JB];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[ni][jb][r] = 0.f;

#pragma unroll 1
    for (int c = 0; c < nc; ++c, buf ^= 1) {
      const bool last = c == nc - 1;
      const bool more = !last || more_tiles;
      if (more) load_z(last ? j0 + BN : j0, last ? 0 : c + 1);
      const _Float16* zb = Zs + buf * ZB;
      f16x8 bh[NI], bl[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        bh[ni] = *reinterpret_cast<const f16x8*>(zb + boff[ni]);
        bl[ni] = *reinterpret_cast<const f16x8*>(zb + boff[ni] + LO);
      }
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(zb + aoff + jb * 32 * 8);
        const f16x8 al = *reinterpret_cast<const f16x8*>(zb + aoff + jb * 32 * 8 + LO);
        // the two small terms first, then the leading one
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) sacc[ni][jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[ni], sacc[ni][jb], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) sacc[ni][jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[ni], sacc[ni][jb], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) sacc[ni][jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ni], sacc[ni][jb], 0, 0, 0);
      }
      if (more) store_z(buf ^ 1);
      __syncthreads();   // chunk c + 1 is staged; every wave is done with this buffer
    }

    mfma_result_fence(sacc);   // the dot products are read on the VALU next (common.hpp)
    if (more_tiles) load_v(j0 + BN);

    // generation and contraction: lane (l31, h) holds dot[j(r, h)][i = l31], j(r, h) = (r & 3) + 8 (r >> 2) + 4 h -- its own B operands of the
    // contraction (kv_gramh.hpp, operand layout)
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      __builtin_amdgcn_sched_barrier(0);   // the operand reads of a block stay in it (hoisted over all four they cost 96 CT registers and spilled)
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
        // rows j(r, h), r = 8 mf + e: 16 mf + 4 h + e (e < 4), 16 mf + 8 + 4 h + e - 4 (e >= 4)
        f32x4 nj[2], ev[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          nj[g] = *reinterpret_cast<const f32x4*>(&Nj[jb * 32 + 16 * mf + 8 * g + 4 * h]);
          if constexpr (EX) ev[g] = *reinterpret_cast<const f32x4*>(&Es[jb * 32 + 16 * mf + 8 * g + 4 * h]);
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          u32x4 kh, kl;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const f32x2 dot = {sacc[ni][jb][8 * mf + 2 * p], sacc[ni][jb][8 * mf + 2 * p + 1]};
            const f32x2 nn = (f32x2){nj[p >> 1][2 * (p & 1)], nj[p >> 1][2 * (p & 1) + 1]} + (f32x2)(ninorm[ni]);
            f32x2 sq = __builtin_elementwise_fma(dot, (f32x2)(-2.f), nn);
            sq = (f32x2){__builtin_fmaxf(sq[0], 0.f), __builtin_fmaxf(sq[1], 0.f)};
            const f32x2 kv = cov_pair_from_sq<KIND>(sq, 0.f, (float)KGH_KSHIFT);
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
    __syncthreads();   // every wave is done with the V planes, the norms and the extra column of this tile
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
