// Fused bilinear derivative:  G = sum_{i,j} W_ij * dK_ij/d(theta),   W = L^T R  (never formed in HBM)
//
// Replaces LinearOperator._bilinear_derivative(left_vecs, right_vecs) on the kernel operator
// (third-party linear_operator) and the dense kernel backward it drives:
// gpytorch/functions/rbf_covariance.py:26-29 and matern_covariance.py:53-56 multiply an n x n
// grad_output (= left @ right^T) with a SAVED n x n dK/dl; the chunked variant is
// gpytorch/lazy/lazy_evaluated_kernel_tensor.py:69-104.
//
// Here each wave forms 32x32 tiles of W^T on the matrix pipe,
//     D[j][i] = sum_c R[c][j] * L[c][i]       (A = R tile, B = L tile; both read straight from the
//                                              probe-major [t][ld] vectors, 128-B coalesced)
// and consumes them in registers: every lane evaluates k and dk/ds for its 16 (j, i) pairs and
// accumulates
//     G[0]     += W_ij * k(s_ij)                      (-> d/d outputscale)
//     G[1 + q] += W_ij * dk/ds(s_ij) * (z_iq - z_jq)^2   (-> d/d lengthscale_q; host applies -2*theta/l_q)
// Algorithmic work: 2 n m t flop on MFMA -- one K*V-equivalent for ALL hyper-parameters (ARD included),
// against (1 + d) K*V-equivalents for a per-parameter contraction.
//
// The W tile is written ONCE, kv_grad_tile below, for every covariance family; a family is a functor that says what it does with one pair (i, j).
#pragma once
#include "common.hpp"

namespace gpamd {

struct GradArgs {
  const float* X1;  // [n][DP]
  const float* X2;  // [m][DP]
  const float* Lt;  // [t][ldl]  left vectors  (index i, with X1)
  const float* Rt;  // [t][ldr]  right vectors (index j, with X2)
  int64_t ldl, ldr;
  int n, m, t;
  int S, jchunk, nrb;  // j split, chunk length (multiple of 64), row blocks of 128
  double* part;        // [nrb*S][F::NG]
  const int* tiles = nullptr;   // far-pair culling (kv_cull.hpp): per unit, the starts of the 64-row j steps it visits (nullptr: all of them)
  int tpc1 = 0;
  float kparam = 0.f;           // shape parameter of the family (PP: the code 4 j + q; PROD: K_A + 4 K_B + 16 D_A, gpamd_kv_grad_param_far_f32); 0 otherwise
};

// The W tile.  One block = 128 rows (4 waves x 32) against one j chunk; a wave stages its L tile and, per 64-row j step, the x_j rows in wave-private
// LDS, forms the two 32 x 32 blocks of W^T on v_mfma_f32_32x32x2_f32 and hands every lane its 32 pairs.  The sums are float over one step, float64
// across steps, then reduced over the wave and the block in a fixed order into part[unit][NG].  The family functor F supplies
//     F::DP            the stride of the prepared rows (a multiple of four)
//     F::NG            the number of block-reduced sums
//     F::TILES         1: the kernel walks a.tiles when there is one (far-pair culling); 0: the family is never culled and visits every step
//     F::ROWS          1: one more sum PER ROW i (not block-reduced): the two half-waves are combined by one lane exchange and every row stores once
//                      per j chunk into fam.rows[s][i]; 0 otherwise
//     fam.begin(a, xi)                 what it reads ONCE before the tile loop (x_i is in registers)
//     fam.pair(w, xi, xj, f[, fr])     the update f[...] += ... of one pair, given W_ij, x_i and the LDS row of x_j (to be read in f32x4 pieces: the
//                                      Matern-1/2 instantiations sit at the register limit); fr: the per-row sum
template <class F>
__device__ __forceinline__ void kv_grad_tile(const GradArgs& a, F fam) {
  constexpr int DP = F::DP, DQ = DP / 4, NG = F::NG;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int th = (a.t + 1) / 2;  // MFMA k-steps (2 probe columns each)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  float* Ls = dyn + (size_t)wave * (2 * th) * 32;              // [2*th][32] this wave's L tile
  float* Xj = dyn + (size_t)4 * (2 * th) * 32 + wave * 64 * DP;  // [64][DP] two j tiles
  __shared__ double red[4][NG];

  const int unit = blockIdx.x;
  const int s = unit / a.nrb, rb = unit - s * a.nrb;
  const int jbeg = s * a.jchunk;
  const int jend = min(a.m, jbeg + a.jchunk);
  const int i0 = rb * 128 + wave * 32;
  const int i = i0 + l31;

  // stage this wave's L tile: Ls[c][ic] = L[c][i0 + ic]  (zero beyond t / n)
  for (int c = h; c < 2 * th; c += 2) {
    float v = 0.f;
    if (c < a.t && i < a.n) v = a.Lt[(int64_t)c * a.ldl + i];
    Ls[c * 32 + l31] = v;
  }
  float xi[DP];
  {
    const int ic = min(i, a.n - 1);
#pragma unroll
    for (int q = 0; q < DQ; ++q) {
      f32x4 v = *reinterpret_cast<const f32x4*>(a.X1 + (int64_t)ic * DP + 4 * q);
      xi[4 * q + 0] = v[0]; xi[4 * q + 1] = v[1]; xi[4 * q + 2] = v[2]; xi[4 * q + 3] = v[3];
    }
  }
  double g[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) g[q] = 0.0;
  [[maybe_unused]] double gi = 0.0;
  fam.begin(a, xi);
  __builtin_amdgcn_wave_barrier();

  const int* tl = F::TILES && a.tiles ? a.tiles + (int64_t)unit * a.tpc1 : nullptr;
  for (int tk = 0, j0; (j0 = tile_start<64>(tl, jbeg, tk)) < jend; ++tk) {
    // stage x_j for the two 32-wide j tiles (wave-private LDS: in-order DS ops, no block barrier)
    {
      const int j = min(j0 + lane, a.m - 1);
#pragma unroll
      for (int q = 0; q < DQ; ++q)
        *reinterpret_cast<f32x4*>(&Xj[lane * DP + 4 * q]) = *reinterpret_cast<const f32x4*>(a.X2 + (int64_t)j * DP + 4 * q);
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const int ja = j0 + l31, jb = j0 + 32 + l31;
    const bool va = ja < jend, vb = jb < jend;
#pragma unroll 4
    for (int c2 = 0; c2 < th; ++c2) {
      const int c = 2 * c2 + h;
      const bool vc = c < a.t;
      const float* rrow = a.Rt + (int64_t)c * a.ldr;
      float ra = (vc && va) ? rrow[ja] : 0.f;
      float rbv = (vc && vb) ? rrow[jb] : 0.f;
      float lb = Ls[c * 32 + l31];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ra, lb, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(rbv, lb, acc1, 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
    float f[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) f[q] = 0.f;
    [[maybe_unused]] float fr = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jr = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float w = half ? acc1[r] : acc0[r];
        if constexpr (F::ROWS) fam.pair(w, xi, &Xj[jr * DP], f, fr);
        else fam.pair(w, xi, &Xj[jr * DP], f);
      }
    }
#pragma unroll
    for (int q = 0; q < NG; ++q) g[q] += (double)f[q];
    if constexpr (F::ROWS) gi += (double)fr;
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (F::ROWS) {
    gi += __shfl_xor(gi, 32, 64);   // the two halves of the wave hold the two column halves of the same 32 rows
    if (h == 0 && i < a.n) fam.rows[(int64_t)s * a.n + i] = gi;
  }
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    double v = wave_sum(g[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (tid < NG) a.part[(int64_t)unit * NG + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// x_j in registers, for the families that index its columns freely
template <int DP>
__device__ __forceinline__ void grad_load_xj(const float* xjrow, float (&xj)[DP]) {
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    f32x4 v = *reinterpret_cast<const f32x4*>(xjrow + 4 * q);
    xj[4 * q + 0] = v[0]; xj[4 * q + 1] = v[1]; xj[4 * q + 2] = v[2]; xj[4 * q + 3] = v[3];
  }
}

// One family KIND over all DP columns (kv_grad_kernel): the two sums of the header comment; ISO: one lengthscale, G[1] alone.
template <int KIND, int DP_, int ISO>
struct GradOne {
  static constexpr int DP = DP_, NG = 1 + DP_, TILES = 1, ROWS = 0;
  float kparam = 0.f;
  PPShape<float> pps = {};   // piecewise polynomial: exponent and coefficients decoded from the shape code ONCE (every q: the singular term of q = 0 included)
  __device__ __forceinline__ void begin(const GradArgs& a, const float (&)[DP]) {
    kparam = a.kparam;
    if constexpr (KIND == KIND_PP) pps = pp_shape(a.kparam);
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    [[maybe_unused]] float df2[DP];
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xjrow + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float df = xi[4 * q + e] - v[e];
        if constexpr (ISO) {
          sq = __builtin_fmaf(df, df, sq);
        } else {
          df2[4 * q + e] = df * df;
          sq += df2[4 * q + e];
        }
      }
    }
    float kv, dk;
    if constexpr (KIND == KIND_PP) {
      pp_cov_dcov(pps, __builtin_amdgcn_sqrtf(sq), kv, dk);
    } else {
      kv = cov_from_sq<KIND>(sq, kparam);
      dk = dcov_dsq<KIND>(sq, kparam);
    }
    f[0] = __builtin_fmaf(w, kv, f[0]);
    const float wd = w * dk;
    if constexpr (ISO) {
      // single lengthscale: sum_q (z_iq - z_jq)^2 = s, one fma instead of DP multiplies + DP fmas
      f[1] = __builtin_fmaf(wd, sq, f[1]);
    } else {
#pragma unroll
      for (int q = 0; q < DP; ++q) f[1 + q] = __builtin_fmaf(wd, df2[q], f[1 + q]);
    }
  }
};

// The PRODUCT of the factors KA (columns [0, D_A)) and KB (the other columns), D_A read from the code at run time -- one compare-and-select per
// dimension, cheap next to the W tile -- always in the per-dimension form (kv_gradp_kernel):
//     G[0]     += W_ij k_A k_B
//     G[1 + q] += W_ij (q < D_A ? k_B dk_A/ds_A : k_A dk_B/ds_B) (z_iq - z_jq)^2
// (Matern-1/2 keeps its r > 1e-15 guard per factor: dcov_dsq.)
template <int KA, int KB, int DP_>
struct GradProd {
  static constexpr int DP = DP_, NG = 1 + DP_, TILES = 1, ROWS = 0;
  int da = DP_;
  __device__ __forceinline__ void begin(const GradArgs& a, const float (&)[DP]) { da = __builtin_amdgcn_readfirstlane(prod_shape_of((int)a.kparam).da); }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    float df2[DP];
    float sq = 0.f, sqb = 0.f;
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xjrow + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float df = xi[4 * q + e] - v[e];
        df2[4 * q + e] = df * df;
        sq += (4 * q + e < da) ? df2[4 * q + e] : 0.f;
        sqb += (4 * q + e < da) ? 0.f : df2[4 * q + e];
      }
    }
    const float kfa = cov_from_sq<KA>(sq), kfb = cov_from_sq<KB>(sqb);
    const float wa = w * kfb * dcov_dsq<KA>(sq), wb = w * kfa * dcov_dsq<KB>(sqb);
    f[0] = __builtin_fmaf(w * kfa, kfb, f[0]);
#pragma unroll
    for (int q = 0; q < DP; ++q) f[1 + q] = __builtin_fmaf(q < da ? wa : wb, df2[q], f[1 + q]);
  }
};

// The ADDITIVE family over the base family KB (kv_grada_kernel), k~ = (1/d) sum_q k'(s_q) with s_q = (z_iq - z_jq)^2 -- per-dimension form:
//     G[0]     += W_ij k~
//     G[1 + q] += W_ij (1/d) dk'/ds(s_q) s_q          (the host's -2 theta / l_q is the same chain rule as for one family: s_q ~ 1 / l_q^2)
// over the d columns that are not padding (NaN in every row: add_col_valid; a select, so no NaN reaches a sum).  Matern-1/2's singular dk/ds at r = 0
// now matters off the diagonal too, on every pair that shares a coordinate: cov_dcov_times_sq forms (dk/ds) s without the quotient (common.hpp).
template <int KB, int DP_>
struct GradAdd {
  static_assert(KB <= KIND_MATERN52, "the additive derivative: one base family");
  static constexpr int DP = DP_, NG = 1 + DP_, TILES = 1, ROWS = 0;
  bool colv[DP_];
  float inv_d = 1.f;
  __device__ __forceinline__ void begin(const GradArgs&, const float (&xi)[DP]) {
    float cnt = 0.f;
#pragma unroll
    for (int q = 0; q < DP; ++q) {
      colv[q] = add_col_valid(xi[q]);
      cnt += colv[q] ? 1.f : 0.f;
    }
    inv_d = 1.0f / cnt;
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    float df2[DP];
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xjrow + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float df = xi[4 * q + e] - v[e];
        df2[4 * q + e] = df * df;
      }
    }
    const float wm = w * inv_d;
    float ks = 0.f;
#pragma unroll
    for (int q = 0; q < DP; ++q) {
      float kq, dq;
      cov_dcov_times_sq<KB>(df2[q], kq, dq);
      ks += colv[q] ? kq : 0.f;
      f[1 + q] = __builtin_fmaf(wm, colv[q] ? dq : 0.f, f[1 + q]);
    }
    f[0] = __builtin_fmaf(wm, ks, f[0]);
  }
};

template <int KIND, int DP, int ISO>
__global__ __launch_bounds__(256) void kv_grad_kernel(GradArgs a) {
  kv_grad_tile(a, GradOne<KIND, DP, ISO>{});
}

template <int KA, int KB, int DP>
__global__ __launch_bounds__(256) void kv_gradp_kernel(GradArgs a) {
  kv_grad_tile(a, GradProd<KA, KB, DP>{});
}

template <int KB, int DP>
__global__ __launch_bounds__(256) void kv_grada_kernel(GradArgs a) {
  kv_grad_tile(a, GradAdd<KB, DP>{});
}

// ---- Spectral-mixture family (kv_directsm.hpp has the formula and the prepared row).  W per pair as above; with tau_j = x_ij - x_jj,
//     e_qj = exp(-2 pi^2 sigma_qj^2 tau_j^2),  g_qj = c_i c_j + s_i s_j (= w^_q cos),  sn_qj = s_i c_j - c_i s_j (= w^_q sin; features again, no per-pair sine),
//     f~_j = sum_q e_qj g_qj,  k~ = prod_j f~_j,  rest~_j = prod_{j' != j} f~_j'
// the 1 + 3 Q d sums, all in the NORMALISED form the prepared features carry (w^ = w / Wsum):
//     G[0]                = sum W k~
//     G[1 + u]            = sum W rest~_j e g            (A~, u = q d + j)
//     G[1 + Q d + u]      = sum W rest~_j e g tau_j^2    (B~)
//     G[1 + 2 Q d + u]    = sum W rest~_j e sn tau_j     (C~)
// The host turns them into the gradients with respect to the raw weights, scales and means (functions.hyper_grads).
struct GradSmArgs {
  GradArgs g;        // part: [nrb*S][1 + 3 Q d]; tiles / kparam unused
  const float* sm;   // [Q d] na[q d + j] = -2 pi^2 sigma_qj^2 log2(e)
};

template <int Q, int DI>
struct GradSm {
  static constexpr int U = Q * DI, DP = (DI + 2 * U + 3) / 4 * 4, NG = 1 + 3 * U, TILES = 0, ROWS = 0;
  const float* sm;
  float na[U];
  __device__ __forceinline__ void begin(const GradArgs&, const float (&)[DP]) {
#pragma unroll
    for (int u = 0; u < U; ++u) na[u] = pp_uniform(sm[u]);
  }
  __device__ __forceinline__ void pair(float w, const float (&xi)[DP], const float* xjrow, float (&f)[NG]) const {
    float xj[DP];
    grad_load_xj(xjrow, xj);
    float ta[U], tb[U], tc[U], fj[DI];
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      const float tau = xi[j] - xj[j], tau2 = tau * tau;
      fj[j] = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int u = q * DI + j, c = DI + 2 * u;
        const float e = __builtin_amdgcn_exp2f(tau2 * na[u]);
        const float gg = __builtin_fmaf(xi[c + 1], xj[c + 1], xi[c] * xj[c]);
        const float sn = __builtin_fmaf(xi[c + 1], xj[c], -xi[c] * xj[c + 1]);
        ta[u] = e * gg;
        tb[u] = ta[u] * tau2;
        tc[u] = e * sn * tau;
        fj[j] += ta[u];
      }
    }
    float kt = fj[0];
#pragma unroll
    for (int j = 1; j < DI; ++j) kt *= fj[j];
    f[0] = __builtin_fmaf(w, kt, f[0]);
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      float rest = w;   // W rest~_j
#pragma unroll
      for (int jj = 0; jj < DI; ++jj)
        if (jj != j) rest *= fj[jj];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int u = q * DI + j;
        f[1 + u] = __builtin_fmaf(rest, ta[u], f[1 + u]);
        f[1 + U + u] = __builtin_fmaf(rest, tb[u], f[1 + U + u]);
        f[1 + 2 * U + u] = __builtin_fmaf(rest, tc[u], f[1 + 2 * U + u]);
      }
    }
  }
};

template <int Q, int DI>
__global__ __launch_bounds__(256) void kv_grad_sm_kernel(GradSmArgs sa) {
  kv_grad_tile(sa.g, GradSm<Q, DI>{sa.sm, {}});
}

// out[q] = sum_u part[u][q]   (1 block of 256 threads; fixed order -> reproducible)
__global__ __launch_bounds__(256) void grad_finalize_kernel(const double* __restrict__ part, int units, int nq,
                                                           float* __restrict__ out) {
  __shared__ double sm[4];
  for (int q = 0; q < nq; ++q) {
    double acc = 0.0;
    for (int u = threadIdx.x; u < units; u += 256) acc += part[(int64_t)u * nq + q];
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) out[q] = (float)acc;
    __syncthreads();
  }
}

}  // namespace gpamd
