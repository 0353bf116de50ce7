// Fused float64 K*V for prepared strides 20 .. 512 (17 .. 512 input dimensions): squared distances in Gram form on the float64 matrix pipe
// (v_mfma_f64_16x16x4_f64), covariance on the VALU, contraction on the same matrix instruction, K never formed.  kv_f64.hpp keeps every x_i of a
// wave in registers (zi[NI][DP], DP <= 16); at 512 columns that would be 256 VGPRs per row tile, so here the dimension count is a RUN-TIME loop over
// chunks of KC = 16 prepared columns staged in LDS, and the per-dimension work is one multiply-add per pair on the matrix pipe -- which on gfx950 runs
// at the VALU's own float64 FMA rate (kv_f64.hpp) but leaves the VALU to the ~35-instruction float64 exp of the covariance.
//
// Accuracy.  s_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j) with the dot product and both norms accumulated as dp-term float64 FMA chains, u = 2^-53:
//     |delta s| <= (dp + 4) u (|z_i| + |z_j|)^2,     |delta k| <= max|dk/ds| (dp + 4) u (|z_i| + |z_j|)^2
// with max|dk/ds| (prepared units, dcov_dsq_f64 at s = 0) = ln 2 (RBF), alpha (RQ), 1/2 (Matern 3/2), 1/6 (Matern 5/2): bounded, so ONE kernel serves
// every extent -- no norm rule, no split operands, no direct-difference twin as float32 needed (kv_wide.hpp).  Matern 1/2 and PP have a cusp in
// r = sqrt(s) at the origin, where an error of u |z|^2 in s becomes sqrt(u) |z| in k: they are not instantiated and stay on row blocks.  The clamp at
// zero matters: coincident points give s = -O(u |z|^2) and the Matern branch takes a square root.
//
// Geometry.  256 threads (4 waves) on a 128-row i block x 64-row j tile; a wave owns 32 i rows (two 16-row tiles) against all 64 j rows (four):
// 8 Gram accumulator tiles of 4 doubles per lane.  Per chunk the workgroup stages the 192 x 16 doubles of both clouds in LDS (row stride 18 doubles:
// the 16 lanes of a 16-byte operand read start 36 words apart = 16 distinct groups of 4 banks); the NEXT chunk's global loads are issued before the
// chunk's MFMAs and held in registers.  Operand layout as at the top of kv_f64.hpp, Gram product G[j][i] = sum_k Zj[j][k] Zi[i][k]:
//     A = Z_j chunk: lane (l15, kq) -> row j0 + l15;   B = Z_i chunk: lane (kq, l15) -> row i0 + l15;   both: column kc + 8 h + 2 kq + e
// for the MFMA (h, e) of the chunk -- the assignment of a chunk's columns to the k index is free as long as A and B agree, so one 16-byte read feeds two
// consecutive MFMAs: 12 reads per lane for 32 MFMAs.  A chunk with <= 8 real columns (the last one of strides 20, 24, 40 ...) issues half of them.
// Norms: after a chunk is staged one thread per staged row adds its squares to a running sum (no pre-pass, no workspace beyond the slabs); the sums
// land in LDS before the covariance step (i rows: on the workgroup's first j tile only).
//
// The contraction needs no data movement.  The Gram D tile leaves lane (kq, l15) with G[j = 4 r + kq][i = l15], r = 0 .. 3; the contraction
// out^T[c][i] = sum_j Vt[c][j] K[j][i] wants its B operand's lane (kq, l15) to hold K[j][i] for k index kq.  So the lane's r-th covariance value IS the B
// operand of one contraction MFMA whose A operand is Vs[c][jb + 4 r + kq]: no lane exchange, no LDS round trip for K, and K is generated once for the
// CT <= 4 column tiles of a launch group (<= 64 columns).  Groups of <= 4 columns contract on the VALU instead (TV = 1 or 4 accumulators per lane, two
// lane exchanges at the end), as kv_f64v_kernel does and for its reason.  Same probe-major layout and split-j partial-slab convention as kv_f64.hpp.
//
// LDS: 27 KB operands + 33 KB V tile (64 columns) + 1.5 KB norms < 64 KB static: two workgroups per CU.
#pragma once
#include "kv_f64.hpp"

namespace gpamd {

constexpr int KW64_BM = 128;               // i rows per workgroup
constexpr int KW64_BN = 64;                // j tile
constexpr int KW64_KC = 16;                // prepared columns per staged chunk
constexpr int KW64_LDZ = KW64_KC + 2;      // padded LDS row of a chunk (doubles)
constexpr int KW64_LDV = KW64_BN + 1;      // padded LDS row of the V tile (kv_f64.hpp KV64_LDV)
constexpr int KW64_MIN_DP = 20, KW64_MAX_DP = 512;
constexpr int KW64_MAX_GROUP = 64;         // columns per launch group (CT <= 4)

struct KvArgsW64 {
  const double* X1;  // [n][dp]
  const double* X2;  // [m][dp]
  const double* Vt;  // [t][ldv]
  double* P;         // [S][t][ldo]
  int64_t ldv, ldo, pstride;
  int n, m, t, dp;
  int S, jchunk, nrb;
  const int* done;
  double kparam;     // shape parameter of the family (RQ: alpha)
};

typedef double f64x2v __attribute__((ext_vector_type(2)));

// Host side (extra_f64_wide.hip, the one unit that instantiates the kernel); called from gpamd_kv_plan_f64 / gpamd_kv_partials_f64
bool kv64w_stride_ok(int dp);
bool kv64w_kind_ok(int kind);
void kv64w_plan(int n, int m, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_doubles);
int kv64w_launch(int kind, double kparam, const double* X1p, int n, const double* X2p, int m, int dp, const double* Vt, int64_t ldv, int t, double* P,
                 int64_t ldo, int S, int jchunk, const int* done, hipStream_t stream);

// CT in 1 .. 4, TV = 0: contraction of 16 CT columns on the matrix pipe;  CT = 0, TV in {1, 4}: contraction of TV columns on the VALU
template <int KIND, int CT, int TV>
__global__ __launch_bounds__(256, 2) void kv_f64w_kernel(KvArgsW64 a) {
  static_assert((TV == 0 && CT >= 1 && CT <= 4) || (CT == 0 && (TV == 1 || TV == 4)), "one contraction flavour");
  constexpr int BM = KW64_BM, BN = KW64_BN, KC = KW64_KC, LDZ = KW64_LDZ, ROWS = BM + BN;
  constexpr int VROWS = CT ? 16 * CT : TV, LDV = CT ? KW64_LDV : BN;
  constexpr int NA = CT ? CT : 1, NV = TV ? TV : 1;
  __shared__ __attribute__((aligned(16))) double Zs[ROWS * LDZ];   // rows 0 .. 127: the i block's chunk, 128 .. 191: the j tile's
  __shared__ __attribute__((aligned(16))) double Vs[VROWS * LDV];
  __shared__ double Ns[ROWS];                                      // |z|^2 of the same rows
  if (a.done && *a.done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;
  const int jend = min(a.m, jbeg + a.jchunk);
  const int i0 = rb * BM;
  const int dp = a.dp;

  // staging: thread -> column pair c2 of rows (tid >> 3) + 32 q;  q < 4: i rows, q = 4, 5: j rows
  const int srow = tid >> 3, c2 = 2 * (tid & 7);
  const double* xi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) xi[q] = a.X1 + (int64_t)min(i0 + srow + 32 * q, a.n - 1) * dp + c2;   // rows beyond n: any finite point (never stored)
  f64x2v pf[6];

  f64x4v acc[2][NA];
  double vacc[2][NV];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
#pragma unroll
    for (int ct = 0; ct < NA; ++ct) acc[it][ct] = (f64x4v){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NV; ++c) vacc[it][c] = 0.0;
  }

  for (int j0 = jbeg; j0 < jend; j0 += BN) {
    const bool first = j0 == jbeg;
    // rows beyond jend: any finite point (their V entries are zero)
    const double* xj0 = a.X2 + (int64_t)min(j0 + srow, a.m - 1) * dp + c2;
    const double* xj1 = a.X2 + (int64_t)min(j0 + srow + 32, a.m - 1) * dp + c2;
    auto fetch = [&](int kc) {
      const bool in = kc + c2 < dp;   // (dp % 4 == 0, c2 even: the pair is inside or outside)
      const f64x2v zero = {0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) pf[q] = in ? *reinterpret_cast<const f64x2v*>(xi[q] + kc) : zero;
      pf[4] = in ? *reinterpret_cast<const f64x2v*>(xj0 + kc) : zero;
      pf[5] = in ? *reinterpret_cast<const f64x2v*>(xj1 + kc) : zero;
    };
    fetch(0);
    f64x4v g[2][4];   // Gram tiles [i tile][j tile]
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) g[it][jt] = (f64x4v){0.0, 0.0, 0.0, 0.0};
    double nsum = 0.0;
    const bool norm_row = tid >= BM ? tid < ROWS : first;   // (wave-uniform)

    for (int kc = 0; kc < dp; kc += KC) {
      __syncthreads();   // the previous chunk's operand reads -- and the previous tile's reads of Vs -- are done
#pragma unroll
      for (int q = 0; q < 6; ++q) *reinterpret_cast<f64x2v*>(&Zs[(srow + 32 * q) * LDZ + c2]) = pf[q];
      if (kc == 0) {
        for (int idx = tid; idx < VROWS * BN; idx += 256) {
          const int c = idx / BN, jj = idx - c * BN;
          const int j = j0 + jj;
          Vs[c * LDV + jj] = (c < a.t && j < jend) ? a.Vt[(int64_t)c * a.ldv + j] : 0.0;
        }
      }
      __syncthreads();
      if (kc + KC < dp) fetch(kc + KC);   // in flight under this chunk's MFMAs
      if (norm_row) {
#pragma unroll
        for (int k = 0; k < KC; k += 2) {
          const f64x2v z = *reinterpret_cast<const f64x2v*>(&Zs[tid * LDZ + k]);
          nsum = fma(z.x, z.x, nsum);
          nsum = fma(z.y, z.y, nsum);
        }
      }
      const int halves = dp - kc > 8 ? 2 : 1;
      for (int h = 0; h < halves; ++h) {
        f64x2v za[4], zb[2];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) za[jt] = *reinterpret_cast<const f64x2v*>(&Zs[(BM + jt * 16 + l15) * LDZ + 8 * h + 2 * kq]);
#pragma unroll
        for (int it = 0; it < 2; ++it) zb[it] = *reinterpret_cast<const f64x2v*>(&Zs[(wave * 32 + it * 16 + l15) * LDZ + 8 * h + 2 * kq]);
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int jt = 0; jt < 4; ++jt) {
            g[it][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[jt].x, zb[it].x, g[it][jt], 0, 0, 0);
            g[it][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[jt].y, zb[it].y, g[it][jt], 0, 0, 0);
          }
      }
    }
    if (norm_row) Ns[tid] = nsum;
    mfma_result_fence(g);   // the Gram results are read by the VALU next (common.hpp)
    __syncthreads();

    double ni[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) ni[it] = Ns[wave * 32 + it * 16 + l15];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jj = jt * 16 + 4 * r + kq;   // D[row = kq + 4 r][col = l15] = G[j = jj][i = l15]
        const double nj = Ns[BM + jj];
        double kv[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const double sq = fmax(0.0, fma(-2.0, g[it][jt][r], ni[it] + nj));
          kv[it] = cov_from_sq_f64<KIND>(sq, a.kparam);
        }
        if constexpr (TV == 0) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const double av = Vs[(ct * 16 + l15) * LDV + jj];
#pragma unroll
            for (int it = 0; it < 2; ++it) acc[it][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kv[it], acc[it][ct], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int c = 0; c < TV; ++c) {
            const double v = Vs[c * LDV + jj];
#pragma unroll
            for (int it = 0; it < 2; ++it) vacc[it][c] = fma(v, kv[it], vacc[it][c]);
          }
        }
      }
  }

  double* Pout = a.P + (int64_t)s * a.pstride;
  if constexpr (TV == 0) {
    mfma_result_fence();   // the accumulators of the last contraction MFMAs are read next (once per workgroup)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = i0 + wave * 32 + it * 16 + l15;
      if (i < a.n) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + kq + 4 * r;
            if (c < a.t) Pout[(int64_t)c * a.ldo + i] = acc[it][ct][r];
          }
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = i0 + wave * 32 + it * 16 + l15;
#pragma unroll
      for (int c = 0; c < TV; ++c) {
        double t0 = vacc[it][c];
        t0 += __shfl_xor(t0, 16, 64);
        t0 += __shfl_xor(t0, 32, 64);
        if (kq == 0 && i < a.n && c < a.t) Pout[(int64_t)c * a.ldo + i] = t0;
      }
    }
  }
}

}  // namespace gpamd
