// Host-side support of libgpamd.so, included by every translation unit that defines entry points: the last-error buffer, launch checks, the
// small geometry helpers and the two compile-time dispatches (covariance family, instantiated dimension).  Host code only: nothing here
// instantiates a kernel by itself.
#pragma once
#include "../../include/gpamd.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <cmath>
#include <type_traits>
#include <utility>

#include "kv_cull.hpp"
#include "kv_dispatch.hpp"

namespace gpamd {

extern thread_local char g_err[512];  // defined in api.hip; what gpamd_last_error() returns

inline int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
// "<what>: <msg>" -- for host code shared by several entry points, so that the message names the one that was called
inline int fail(int code, const char* what, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, msg);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, what, hipGetErrorString(e));
  return 0;
}

// compute units of the current device (256 without one); one cached value for the library
inline int num_cus() {
  static const int cus = [] {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
      return p.multiProcessorCount;
    return 256;
  }();
  return cus;
}

// workgroups (= partial sums) per column of the vector kernels: 1024 elements each, at most `cap` (CG_MAXNB, LZ_MAXNB)
inline unsigned col_blocks(int n, int cap) {
  long nb = ((long)n + 1023) / 1024;
  if (nb < 1) nb = 1;
  if (nb > cap) nb = cap;
  return (unsigned)nb;
}

// factor of prep_points: z = (x - shift) * prep_coef / lengthscale (common.hpp, "Covariance families")
template <typename T>
T prep_coef(int kind, T kparam) {
  switch (kind) {
    case GPAMD_RBF: return std::sqrt(T(0.5) * T(1.4426950408889634));  // exp(-0.5 s) = exp2(-(0.5 log2 e) s)
    case GPAMD_MATERN12: return T(1);
    case GPAMD_MATERN32: return std::sqrt(T(3));
    case GPAMD_MATERN52: return std::sqrt(T(5));
    case GPAMD_RQ: return T(1) / std::sqrt(T(2) * kparam);   // (1 + |x - x'|^2 / (2 alpha l^2))^-alpha = (1 + |z - z'|^2)^-alpha
    case GPAMD_PP: return T(1);                              // support radius = one lengthscale
    case GPAMD_PROD: return prep_coef<T>(prod_shape_of((int)kparam).ka, T(0));   // the first factor's; the second's: prep_coef(shape.kb, 0)
    case GPAMD_ADD: return prep_coef<T>((int)kparam, T(0));                       // the base family's, for every column
  }
  return T(0);
}

// The shape parameter of a parametrised family as the entry points accept it, or the message they fail with (GPAMD_EINVAL).  PP: the code 4 j + q
// with q in 0..3 and j >= q + 1 (j = floor(D / 2) + q + 1 for D >= 0 input dimensions), an integer.  PROD: the code K_A + 4 K_B + 16 D_A in canonical
// order (include/gpamd.h); `d` = D_A + D_B where the entry point knows it (0: it sees the padded stride only and checks what the code alone says).
// ADD: the base family's id 0..3, and d in 2..8 where the entry point knows it
inline const char* kparam_error(int kind, double kparam, int d = 0) {
  if (kind == GPAMD_RQ && !(kparam > 0.0)) return "the rational-quadratic shape parameter alpha must be positive";
  if (kind == GPAMD_PP) {
    const int code = (int)kparam;
    if (!(kparam >= 0.0 && kparam < 1024.0) || (double)code != kparam || (code >> 2) < (code & 3) + 1)
      return "the piecewise-polynomial shape code must be 4 j + q with q in 0..3 and j >= q + 1";
  }
  if (kind == GPAMD_PROD) {
    static const char* const bad =
        "the product code must be K_A + 4 K_B + 16 D_A with K_A <= K_B <= 3 (family ids), not both RBF, 1 <= D_A <= 3, 1 <= d - D_A <= 3, and "
        "D_A <= d - D_A for equal families";
    const int code = (int)kparam;
    if (!(kparam >= 0.0 && kparam < 64.0) || (double)code != kparam) return bad;
    const ProdShape c = prod_shape_of(code);
    if (c.ka > c.kb || c.kb == 0 || c.da < 1) return bad;   // (code < 64: D_A <= 3)
    if (d > 0 && (d - c.da < 1 || d - c.da > 3 || (c.ka == c.kb && c.da > d - c.da))) return bad;
  }
  if (kind == GPAMD_ADD) {
    if (!(kparam == 0.0 || kparam == 1.0 || kparam == 2.0 || kparam == 3.0))
      return "the additive family's kparam must be the base family's id: 0 (RBF), 1, 2 or 3 (Matern 1/2, 3/2, 5/2)";
    if (d != 0 && (d < 2 || d > 8)) return "the additive family takes d in 2..8";
  }
  return nullptr;
}

// Family dispatch: calls f(std::integral_constant<int, KIND_*>) for the ABI's GPAMD_* `kind` when the caller's mask accepts it (f is
// instantiated for the accepted families only); false otherwise.
constexpr unsigned kind_bit(int kind) { return 1u << kind; }
constexpr unsigned KINDS_ALL = kind_bit(GPAMD_RBF) | kind_bit(GPAMD_MATERN12) | kind_bit(GPAMD_MATERN32) | kind_bit(GPAMD_MATERN52) | kind_bit(GPAMD_RQ) |
                               kind_bit(GPAMD_PP);
constexpr unsigned KINDS_GRAM = KINDS_ALL & ~kind_bit(GPAMD_MATERN12);   // the quadratic expansion of the squared distance: not for Matern nu = 1/2
constexpr unsigned KINDS_NO_RQ = KINDS_ALL & ~kind_bit(GPAMD_RQ);   // the direct-difference derivative kernel returns no shape-parameter sum
template <unsigned ACCEPT, int GK, int KK, typename F>
bool try_kind(int kind, F& f) {
  if constexpr ((ACCEPT & kind_bit(GK)) != 0) {
    if (kind == GK) {
      f(std::integral_constant<int, KK>{});
      return true;
    }
  }
  return false;
}
// ... and the product of two of them where the kernel decodes the factors itself (misc_kernels.hpp cov_pair): rows, dense blocks, diagonals, pivoted Cholesky
// ... and the additive family, whose point-wise covariance is a loop over the columns of the two rows
constexpr unsigned KINDS_POINTWISE = KINDS_ALL | kind_bit(GPAMD_PROD) | kind_bit(GPAMD_ADD);
// ... and the masks of the entry points that check `kind` before they dispatch: explicit lists (kinds 7 and 9, the spectral mixture and the Newton-Girard additive family, have their own entry points)
constexpr unsigned KINDS_PREP = KINDS_POINTWISE;                      // gpamd_prep_points_f32, gpamd_kv_f32
constexpr unsigned KINDS_KV = KINDS_POINTWISE | kind_bit(GPAMD_SM) | kind_bit(GPAMD_GIBBS);   // gpamd_kv_plan, the shared K * V launch code (kinds 9, 11 and 12 reach that code from their own entry points only)
constexpr unsigned KINDS_GRAD_PARAM = KINDS_NO_RQ | kind_bit(GPAMD_PROD) | kind_bit(GPAMD_ADD);   // gpamd_kv_grad_param_far_f32
inline bool kind_accepted(int kind, unsigned mask) { return kind >= 0 && kind < 32 && (mask & kind_bit(kind)) != 0; }
template <unsigned ACCEPT = KINDS_ALL, typename F>
bool with_kind(int kind, F&& f) {
  return try_kind<ACCEPT, GPAMD_RBF, KIND_RBF>(kind, f) || try_kind<ACCEPT, GPAMD_MATERN12, KIND_MATERN12>(kind, f) ||
         try_kind<ACCEPT, GPAMD_MATERN32, KIND_MATERN32>(kind, f) || try_kind<ACCEPT, GPAMD_MATERN52, KIND_MATERN52>(kind, f) ||
         try_kind<ACCEPT, GPAMD_RQ, KIND_RQ>(kind, f) || try_kind<ACCEPT, GPAMD_PP, KIND_PP>(kind, f) ||
         try_kind<ACCEPT, GPAMD_PROD, KIND_PROD>(kind, f) || try_kind<ACCEPT, GPAMD_ADD, KIND_ADD>(kind, f);
}

// Factor dispatch of the product family: calls f(integral_constant K_A, integral_constant K_B) for the nine canonical pairs (K_A <= K_B, not both RBF)
template <int KA, int KB, typename F>
bool try_pair(int ka, int kb, F& f) {
  if (ka == KA && kb == KB) {
    f(std::integral_constant<int, KA>{}, std::integral_constant<int, KB>{});
    return true;
  }
  return false;
}
template <typename F>
bool with_prod_pair(int ka, int kb, F&& f) {
  return try_pair<0, 1>(ka, kb, f) || try_pair<0, 2>(ka, kb, f) || try_pair<0, 3>(ka, kb, f) || try_pair<1, 1>(ka, kb, f) || try_pair<1, 2>(ka, kb, f) ||
         try_pair<1, 3>(ka, kb, f) || try_pair<2, 2>(ka, kb, f) || try_pair<2, 3>(ka, kb, f) || try_pair<3, 3>(ka, kb, f);
}

// Dimension dispatch: calls f(std::integral_constant<int, D>) for the instantiated dimension D == dk (dk = kv_kernel_dims(d), kv_dispatch.hpp) up
// to MAXD (f is instantiated for those only); false otherwise.  (Listed largest first: hipcc then emits the kernels of a unit in ascending D, as the
// switch ladders this replaces did, and its code object stays byte-comparable with earlier builds.)
template <int MAXD, int D, typename F>
bool try_dim(int dk, F& f) {
  static_assert(kv_kernel_dims(D) == D, "the instantiated dimensions are the fixed points of kv_kernel_dims");
  if constexpr (D <= MAXD) {
    if (dk == D) {
      f(std::integral_constant<int, D>{});
      return true;
    }
  }
  return false;
}
template <int MAXD, typename F, int... D>
bool with_dim_of(int dk, F& f, std::integer_sequence<int, D...>) {
  return (try_dim<MAXD, D>(dk, f) || ...);
}
template <int MAXD = KV_MAX_DIM, typename F>
bool with_dim(int dk, F&& f) {
  return with_dim_of<MAXD>(dk, f, std::integer_sequence<int, 32, 24, 20, 16, 12, 10, 8, 6, 5, 4, 3, 2, 1>{});
}

// Arguments of cull_list_kernel (kv_cull.hpp) for row blocks of bm and tiles of bn points; a unit's list holds jchunk / bn + 1 entries
inline CullArgs cull_args(const float* row_centres, const float* row_radii, const float* tile_centres, const float* tile_radii, int* tiles, int n, int m,
                          int dp, int bm, int bn, int nrb, int jchunk, float sq_cutoff, const int* done) {
  CullArgs c;
  c.rc = row_centres; c.rr = row_radii; c.tc = tile_centres; c.tr = tile_radii;
  c.tiles = tiles; c.tpc1 = jchunk / bn + 1;
  c.n = n; c.m = m; c.dp = dp; c.bm = bm; c.bn = bn; c.nrb = nrb; c.jchunk = jchunk;
  c.sq_cut = sq_cutoff; c.done = done;
  return c;
}

}  // namespace gpamd
