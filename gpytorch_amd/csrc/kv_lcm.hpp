// Fused product of the linear model of coregionalisation, (sum_q theta_q K_q (x) B_q) V = sum_q K_q (V_mat (theta_q B_q)^T): Q latent covariances over ONE
// cloud, each with its own family and lengthscales, every one with its own T x T task covariance (gpytorch/kernels/lcm_kernel.py:56-60 sums one
// gpytorch/kernels/multitask_kernel.py:46-61 Kronecker operator per base kernel).  The Q terms accumulate into the same output tile, so the product is ONE
// contraction whose K dimension is Q times as long, [K_1 | ... | K_Q] [W_1; ...; W_Q], W_q = V_mat (theta_q B_q)^T: one set of accumulators, the x_j tile
// staged once, the coordinate differences of a pair formed once, the output written once -- where Q launches of kv_directh_kernel stage, difference,
// write slabs, reduce and add Q times.
//
// It is kv_directh_body.inc's design (4 waves x NI row tiles, the 128-j LDS tile with double-buffered x_j, hi/lo operands on v_mfma_f32_32x32x16_f16 with
// three terms per block, the 2^12 range shift, mfma_result_fence, slabs and the done flag) with a body of its own, because
//   * the V planes in LDS are [Q][32 columns][hi, lo]: 17.4 KB per member, 70 KB at Q = 4 (+ 2 x 2 KB of x_j at d = 4): two workgroups per CU;
//   * the prepared rows are the centred UNSCALED points (stride 4); a device block carries, per member, its family id and the d weights
//     w_qk = (coef_family / l_qk)^2.  A half-block of pairs computes its d squared differences per pair ONCE (dsq, 8 d registers), then every member
//     takes s_q = sum_k w_qk dsq_k (d multiply-adds from scalar registers) and the radial function of ITS family -- a wave-uniform value, so a scalar
//     branch around cov_pair_from_sq: one instantiation per (D, Q, NI), not 4^Q bodies;
//   * the pipeline unit is one HALF block of one member, (jb, ni, mf, q) with q innermost: its three MFMAs into acc[ni] cover the generation of the
//     next unit's B operands -- member q + 1 of the same pairs, or member 0 of the next half / row tile / j block / LDS tile, whose dsq is formed then.
//     The A operands (two ds_read_b128) are fetched one unit ahead;
//   * columns are (probe, task) pairs, c = probe T + task, floor(32 / T) whole probes per launch group, and the epilogue writes the INTERLEAVED
//     layout out[probe][i T + task] straight into the slabs: kv_reduce then sums slabs of "probes" columns of n T entries, and its diagonal epilogue
//     takes the interleaved noise vector as it is.  No extra VALU column.
// Pre-pass (lcm_colmax_kernel, lcm_mix_split_kernel): reads the interleaved right-hand side [probes][m T] and forms all Q T mixed columns of a probe
// in registers, the column's power-of-two scale shared by its Q members (they meet in one accumulator), the f16 planes in the k-slot order of the MFMA
// A operand (kv_gramh.hpp).  It replaces the de-interleave, the einsum and Q split passes of the Kronecker form.
// The summation order is fixed: two launches give the same bits.
#pragma once
#include "kv_directh.hpp"

namespace gpamd {

constexpr int KLC_MAX_DIM = 4;        // input dimensions (the prepared stride)
constexpr int KLC_MAX_MEMBERS = 4;    // Q
constexpr int KLC_MIN_TASKS = 2, KLC_MAX_TASKS = 8;   // T
constexpr int KLC_COLS = 32;          // columns per launch group: floor(32 / T) whole probes
// the parameter block, float32, KLC_MEMBER floats per member: [0] family id 0..3 (RBF, Matern 1/2, 3/2, 5/2)  [1..4] w_qk, zero beyond d
// [8 + 8 tau + tau'] theta_q B_q[tau][tau'], zero beyond T
constexpr int KLC_MEMBER = 8 + KLC_MAX_TASKS * KLC_MAX_TASKS;
constexpr int klc_ni(bool small) { return small ? 1 : 2; }   // the row-tile rule of the direct-difference kernels (kdh_ni at one column tile)
constexpr int klc_probes(int tasks) { return KLC_COLS / tasks; }

struct KvLcmArgs {
  KvArgs a;               // X1, X2: centred unscaled points, stride 4; t: the columns of this group (probes x T); P: the interleaved slabs; Vt unused
  const _Float16* Vh;     // [Q][32][ldh] split planes of the mixed columns, permuted k-slot order, zero beyond m
  const _Float16* Vl;
  int64_t ldh;
  const float* colmul;    // [32] per-column output multiplier
  const float* par;       // the parameter block
  int tasks;              // T
};

// The radial function of a member whose family is a wave-uniform run-time value: a scalar branch around cov_pair_from_sq (the 2^12 shift in every exponent)
__device__ __forceinline__ f32x2 lcm_pair_from_sq(int fam, f32x2 s) {
  constexpr float KS = (float)KGH_KSHIFT;
  switch (fam) {
    case KIND_RBF: return cov_pair_from_sq<KIND_RBF>(s, 0.f, KS);
    case KIND_MATERN12: return cov_pair_from_sq<KIND_MATERN12>(s, 0.f, KS);
    case KIND_MATERN32: return cov_pair_from_sq<KIND_MATERN32>(s, 0.f, KS);
    default: return cov_pair_from_sq<KIND_MATERN52>(s, 0.f, KS);
  }
}

template <int D, int Q, int NI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void kv_lcm_kernel(KvLcmArgs ka) {
  static_assert(D >= 1 && D <= KLC_MAX_DIM && Q >= 1 && Q <= KLC_MAX_MEMBERS, "1 <= D <= 4, 1 <= Q <= 4");
  constexpr int NW = 4, NT = 64 * NW, DP = 4;
  constexpr int BN = KGH_BN, LDH = KGH_LDH, TC = KLC_COLS, ROWS = Q * TC;
  constexpr int XFS = D * BN;   // floats of one x_j buffer
  const KvArgs& a = ka.a;
  __shared__ __attribute__((aligned(16))) _Float16 Vhs[ROWS * LDH];   // [q][c][j]
  __shared__ __attribute__((aligned(16))) _Float16 Vls[ROWS * LDH];
  __shared__ __attribute__((aligned(16))) float Xf[2 * XFS];          // [buf][k][j]

  if (a.done && *a.done) return;
  float negone;   // -1.0f the optimiser cannot see through (gen_b, kv_gramh.hpp)
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(negone));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;                  // multiple of BN
  const int jend = min(a.m, jbeg + a.jchunk);
  const int ibase = rb * (NW * NI * 32) + wave * (NI * 32);

  // per member: family and metric weights, wave-uniform (scalar registers)
  int fam[Q];
  float w[Q][D];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    fam[q] = __builtin_amdgcn_readfirstlane((int)ka.par[q * KLC_MEMBER]);
#pragma unroll
    for (int k = 0; k < D; ++k) w[q][k] = pp_uniform(ka.par[q * KLC_MEMBER + 1 + k]);
  }

  float zi[NI][D];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int i = min(ibase + ni * 32 + l31, a.n - 1);
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.X1 + (int64_t)i * DP);
#pragma unroll
    for (int e = 0; e < D; ++e) zi[ni][e] = v[e];
  }

  f32x16 acc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

  // x_j rows of the tile starting at j0 -> buffer `buf`, transposed (rows beyond jend: zero -> a finite k against V = 0)
  f32x4 xz = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int j0) {
    if (tid < BN) {
      const int j = j0 + tid;
      xz = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (j < jend) xz = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * DP);
    }
  };
  auto store_x = [&](int buf) {
    if (tid < BN) {
#pragma unroll
      for (int k = 0; k < D; ++k) Xf[buf * XFS + k * BN + tid] = xz[k];
    }
  };

  // Generation.  gen_dsq: the squared coordinate differences of the 8 pairs (4 packed) of half mf of block jb against row tile ni -- once for all
  // members.  gen_a: member q's squared distance of pair p, its covariance, the packed hi word;  gen_b: lo = K - hi, the packed lo word (kv_gramh.hpp)
  f32x2 dsq[4][D];
  auto gen_dsq = [&](int buf, int jb, int mf, int ni) {
#pragma unroll
    for (int qd = 0; qd < 2; ++qd)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const f32x4 zq = *reinterpret_cast<const f32x4*>(&Xf[buf * XFS + k * BN + jb + 16 * mf + 8 * qd + 4 * h]);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const f32x2 df = (f32x2){zi[ni][k], zi[ni][k]} - (f32x2){zq[2 * e], zq[2 * e + 1]};
          dsq[2 * qd + e][k] = df * df;
        }
      }
  };
  auto gen_a = [&](int q, int p, f32x2& kv, u32x4& bh) {
    f32x2 s2 = dsq[p][0] * (f32x2)(w[q][0]);
#pragma unroll
    for (int k = 1; k < D; ++k) s2 = __builtin_elementwise_fma(dsq[p][k], (f32x2)(w[q][k]), s2);
    kv = lcm_pair_from_sq(fam[q], s2);
    bh[p] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(kv[0], kv[1]));
  };
  auto gen_b = [&](const f32x2& kv, int p, uint32_t hiw, u32x4& bl) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 hv = __builtin_bit_cast(f16x2, hiw);
    const float l0 = __builtin_fmaf((float)hv[0], negone, kv[0]);
    const float l1 = __builtin_fmaf((float)hv[1], negone, kv[1]);
    bl[p] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(l0, l1));
  };
  // the A operands of unit (jb, mf, q): this lane's column l31 of member q, k-slots 8 h .. 8 h + 7 of half mf
  auto load_a = [&](int jb, int mf, int q, f16x8& ah, f16x8& al) {
    const int o = (q * TC + l31) * LDH + jb + 16 * mf + 8 * h;
    ah = *reinterpret_cast<const f16x8*>(&Vhs[o]);
    al = *reinterpret_cast<const f16x8*>(&Vls[o]);
  };

  // prologue: x rows of the first tile, B operands of its first unit
  load_x(jbeg);
  store_x(0);
  __syncthreads();
  u32x4 bh, bl;
  gen_dsq(0, 0, 0, 0);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    f32x2 kv;
    gen_a(0, p, kv, bh);
    gen_b(kv, p, bh[p], bl);
  }

  constexpr int VQ = ROWS * (BN / 8) / NT;   // 16-byte chunks per thread and plane (= 2 Q)
  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += BN, buf ^= 1) {
    __syncthreads();   // every wave is done with the V planes of the previous tile and with Xf[buf ^ 1]
    {
      load_x(j0 + BN);   // past the end of the chunk: zero rows (the last unit's look-ahead generation must stay finite)
      store_x(buf ^ 1);
      const int64_t jc = min((int64_t)j0, ka.ldh - BN);
#pragma unroll
      for (int rr = 0; rr < VQ; ++rr) {
        const int idx = tid + NT * rr;
        const int c = idx / (BN / 8), ch = idx % (BN / 8);
        const int64_t off = (int64_t)c * ka.ldh + jc + 8 * ch;
        const u32x4 ph = *reinterpret_cast<const u32x4*>(ka.Vh + off);
        const u32x4 pl = *reinterpret_cast<const u32x4*>(ka.Vl + off);
        *reinterpret_cast<u32x4*>(&Vhs[c * LDH + 8 * ch]) = ph;
        *reinterpret_cast<u32x4*>(&Vls[c * LDH + 8 * ch]) = pl;
      }
    }
    __syncthreads();

    f16x8 ah, al;
    load_a(0, 0, 0, ah, al);
#pragma unroll 1
    for (int jb = 0; jb < BN; jb += 32) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            // the next unit: member q + 1 of these pairs, else member 0 of the next half, row tile or block -- of the NEXT LDS tile after the last
            // block (its x rows are staged already; past the end of the chunk they are zero rows and the result is never used)
            const bool newpairs = (q == Q - 1);
            const int qn = newpairs ? 0 : q + 1;
            const int mfn = newpairs ? (mf ^ 1) : mf;
            const bool newtile = newpairs && mf == 1;
            const int nin = newtile ? (ni == NI - 1 ? 0 : ni + 1) : ni;
            const bool wrap = newtile && ni == NI - 1;
            const int jbn = wrap ? ((jb + 32) & (BN - 1)) : jb;
            const int bufn = (wrap && jb == BN - 32) ? (buf ^ 1) : buf;
            const f16x8 bhv = __builtin_bit_cast(f16x8, bh);
            const f16x8 blv = __builtin_bit_cast(f16x8, bl);
            u32x4 bhn, bln;
            f16x8 ahn, aln;
            f32x2 kv[4];
            __builtin_amdgcn_sched_barrier(0);
            load_a(jbn, mfn, qn, ahn, aln);   // (after the last block of a tile: a harmless re-read of block 0; the tile loop reloads)
#pragma unroll
            for (int term = 0; term < 3; ++term) {
              // the two small terms first, then the leading one
              acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 0 ? al : ah, term == 1 ? blv : bhv, acc[ni], 0, 0, 0);
              if (term == 0 && newpairs) gen_dsq(bufn, jbn, mfn, nin);
              // half-chunk u = 2 p + (0: gen_a, 1: gen_b); this MFMA's share:  a0 b0 a1 | b1 a2 b2 | a3 b3   (kv_gramh.hpp, one column tile)
              constexpr int U3[4] = {0, 3, 6, 8};
#pragma unroll
              for (int u = U3[term]; u < U3[term + 1]; ++u) {
                if ((u & 1) == 0) gen_a(qn, u >> 1, kv[u >> 1], bhn);
                else gen_b(kv[u >> 1], u >> 1, bhn[u >> 1], bln);
              }
              __builtin_amdgcn_sched_barrier(0);
            }
            bh = bhn; bl = bln; ah = ahn; al = aln;
          }
    }
  }

  mfma_result_fence();   // the accumulators of the last contraction MFMAs are read next (common.hpp; once per workgroup)
  // epilogue: column c = probe T + task of row i goes to out[probe][i T + task] of this chunk's slab
  float* Pout = a.P + (int64_t)s * a.pstride;
  const int T = ka.tasks;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int i = ibase + ni * 32 + l31;
    if (i < a.n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (c < a.t) {
          const int pr = c / T, tau = c - pr * T;
          Pout[(int64_t)pr * a.ldo + (int64_t)i * T + tau] = acc[ni][r] * ka.colmul[c];
        }
      }
    }
  }
}

// ---- pre-pass.  One thread per (probe of the group, 8 positions): it reads the 8 T interleaved values of its points and forms
// W_q[tau] = sum_tau' (theta_q B_q)[tau][tau'] v[tau'] for all members in registers.
// colmax[c] = bits of max over members and positions of |W_q[c]|, c = probe T + tau (non-negative floats order like unsigned integers); zeroed by
// lcm_clear_kernel
__global__ void lcm_clear_kernel(unsigned* colmax, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) colmax[i] = 0u;
}

template <int T>
__device__ __forceinline__ void lcm_mix(const float* par, int q, const float (&v)[T], float (&wq)[T]) {
#pragma unroll
  for (int tau = 0; tau < T; ++tau) {
    float sum = 0.f;
#pragma unroll
    for (int tp = 0; tp < T; ++tp) sum = __builtin_fmaf(par[q * KLC_MEMBER + 8 + 8 * tau + tp], v[tp], sum);
    wq[tau] = sum;
  }
}

// Vi: this group's probes, [probes][ldv] interleaved (entry j T + tau); grid (position blocks, probes)
template <int T>
__global__ __launch_bounds__(256) void lcm_colmax_kernel(const float* Vi, int64_t ldv, int m, int Q, const float* par, unsigned* colmax, const int* done) {
  if (done && *done) return;
  const int pr = blockIdx.y;
  const float* src = Vi + (int64_t)pr * ldv;
  float mx[T];
#pragma unroll
  for (int tau = 0; tau < T; ++tau) mx[tau] = 0.f;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += 256 * gridDim.x) {
    float v[T], wq[T];
#pragma unroll
    for (int tau = 0; tau < T; ++tau) v[tau] = src[(int64_t)j * T + tau];
    for (int q = 0; q < Q; ++q) {
      lcm_mix<T>(par, q, v, wq);
#pragma unroll
      for (int tau = 0; tau < T; ++tau) mx[tau] = fmaxf(mx[tau], fabsf(wq[tau]));
    }
  }
#pragma unroll
  for (int tau = 0; tau < T; ++tau) {
    float x = mx[tau];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    if ((threadIdx.x & 63) == 0 && x > 0.f) atomicMax(&colmax[pr * T + tau], __float_as_uint(x));
  }
}

// planes[q 32 + c][16 g + 8 h + e] = split(scale_c W_q[c][16 g + (e & 3) + 8 (e >> 2) + 4 h]) with ONE scale per column c for its Q members; positions
// >= m and the columns beyond probes T are zero.  One thread per 8 positions and probe: one 16-byte store per plane, member and task
template <int T>
__global__ __launch_bounds__(256) void lcm_mix_split_kernel(const float* Vi, int64_t ldv, int m, int probes, int Q, const float* par, _Float16* Vh,
                                                            _Float16* Vl, int64_t ldh, const unsigned* colmax, float* colmul, const int* done) {
  if (done && *done) return;
  const int pr = blockIdx.y;
  const int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x;   // chunk of 8 positions
  if (8 * ch >= ldh) return;
  float scale[T];
#pragma unroll
  for (int tau = 0; tau < T; ++tau) {
    scale[tau] = 1.0f;
    const float mx = __uint_as_float(colmax[pr * T + tau]);
    if (mx > 0.f && mx < 3.0e38f) {
      int ex;
      (void)frexpf(mx, &ex);                    // mx = f 2^ex, f in [0.5, 1)
      int sh = KGH_VEXP - ex;
      sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
      scale[tau] = ldexpf(1.0f, sh);
    }
    if (ch == 0) colmul[pr * T + tau] = ldexpf(1.0f, -KGH_KSHIFT) / scale[tau];
  }
  const int g = (int)(ch >> 1), hh = (int)(ch & 1);
  const int ja = 16 * g + 4 * hh;
  const float* src = Vi + (int64_t)pr * ldv;
  float v[8][T];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int j = ja + (e & 3) + 8 * (e >> 2);
#pragma unroll
    for (int tau = 0; tau < T; ++tau) v[e][tau] = j < m ? src[(int64_t)j * T + tau] : 0.f;
  }
  for (int q = 0; q < Q; ++q) {
    f16x8 hi[T], lo[T];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float wq[T];
      lcm_mix<T>(par, q, v[e], wq);
#pragma unroll
      for (int tau = 0; tau < T; ++tau) {
        _Float16 x, y;
        f16_split(wq[tau] * scale[tau], x, y);
        hi[tau][e] = x;
        lo[tau][e] = y;
      }
    }
#pragma unroll
    for (int tau = 0; tau < T; ++tau) {
      const int64_t off = (int64_t)(q * KLC_COLS + pr * T + tau) * ldh + 8 * ch;
      *reinterpret_cast<f16x8*>(Vh + off) = hi[tau];
      *reinterpret_cast<f16x8*>(Vl + off) = lo[tau];
    }
    if (pr == 0) {   // the columns no probe of the group fills (32 - probes T < T of them, and those of the probes a short last group lacks)
      const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int c = probes * T; c < KLC_COLS; ++c) {
        const int64_t off = (int64_t)(q * KLC_COLS + c) * ldh + 8 * ch;
        *reinterpret_cast<f16x8*>(Vh + off) = zero;
        *reinterpret_cast<f16x8*>(Vl + off) = zero;
      }
    }
  }
}

}  // namespace gpamd
