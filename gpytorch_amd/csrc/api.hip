// extern "C" entry points of libgpamd.so (see include/gpamd.h for the contract and the reference
// interfaces each one replaces).  gfx950 only; no torch types, no CPU fallbacks.
#include "../../include/gpamd.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cg_host.hpp"
#include "kv_dispatch.hpp"
#include "kv_cull.hpp"
#include "kv_valu.hpp"
#include "kv_gramv.hpp"
#include "kv_gram4.hpp"
#include "kv_gram16.hpp"
#include "kv_vsplit.hpp"
#include "kv_directh.hpp"
#include "kv_directp.hpp"
#include "kv_directadd.hpp"
#include "kv_directsm.hpp"
#include "kv_directng.hpp"
#include "kv_directps.hpp"
#include "kv_directgibbs.hpp"
#include "kv_directham.hpp"
#include "misc_kernels.hpp"

using namespace gpamd;

namespace gpamd {
thread_local char g_err[512] = "";  // shared by every translation unit of the library (gpamd_last_error)
}

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The point-wise entry points (rows, dense blocks, diagonals, pivoted Cholesky) see the padded stride only: for the product family, what the code alone
// says, a stride of 4 or 8 (d <= 6) and the first factor's columns inside it; nullptr for every other family (their kparam is not validated here)
const char* pointwise_error(int kind, double kparam, int dp) {
  if (kind != GPAMD_ADD && kind != GPAMD_PROD) return nullptr;
  if (const char* bad = kparam_error(kind, kparam)) return bad;
  const bool stride_ok = dp == 4 || dp == 8;   // (additive, d in 2..8: the padding columns hold NaN and are not counted)
  if (kind == GPAMD_ADD) return stride_ok ? nullptr : "the additive family takes points prepared with stride 4 or 8 (d in 2..8)";
  return (stride_ok && prod_shape_of((int)kparam).da < dp) ? nullptr : "the product family takes points prepared with stride 4 or 8 (d = D_A + D_B <= 6)";
}

// column-tile variant for t columns: valu (t <= 8) or mfma CT/EX
struct KvVariant {
  bool valu;
  int tpad;    // valu: 1,2,4,8
  int ct, ex;  // mfma
  int g4;      // > 0: kv_gram4 with this many column groups of four (2, 3, 6); 16 / 17: kv_gram16 without / with EX
  bool split;  // kv_gramh: contraction of hi/lo-split operands on the f16 matrix pipe (ct, ex as for mfma)
  int ni;      // kv_gramh: 32-row tiles per wave
  bool gram;   // the selected kernel forms the squared distances by the quadratic expansion (false: direct differences)
  bool direct; // with split: kv_directh (direct differences + split contraction; ct, ex as for mfma, ct <= 2)
  int bm;      // rows per workgroup
  int bn;      // j tile
};

typedef const void* (*Ptr4)(int, int, int, int);   // a family's kernel lookup
bool gram_ok(int kind, int flags);

// A family that travels with a device block comes through its own entry point, which hands block and kernel code to the shared launch code.  Spectral
// mixture (kv_directsm.hpp): the parameter block, code 4 Q + d; the `d` of the shared host code below is then the WIDTH d + 2 Q d of its prepared rows.
// Newton-Girard additive (kv_directng.hpp): the weight block, code base + 4 full (full: the kernel with degree cap d, else min(d, 3)); `d` as for the additive family
// Hamming (kv_directham.hpp): no block -- its two shape parameters 1 / alpha and beta travel BY VALUE in the eight bytes where the others keep the pointer;
// code = the prepared width, which is its `d` too
struct BlockLaunch {
  const float* block;
  int code;
  float tail[2] = {0.f, 0.f};   // by-value parameters of a family without a block
};
// (both blocks ride behind KvhArgs as ONE pointer: the shared launch code fills a KvSmArgs for either family)
static_assert(sizeof(KvNgArgs) == sizeof(KvSmArgs) && offsetof(KvNgArgs, w) == offsetof(KvSmArgs, sm), "KvNgArgs and KvSmArgs share their layout");
static_assert(sizeof(KvHamArgs) == sizeof(KvSmArgs) && offsetof(KvHamArgs, inv_alpha) == offsetof(KvSmArgs, sm) && sizeof(BlockLaunch::tail) == sizeof(const float*),
              "KvHamArgs keeps its two floats where KvSmArgs keeps its pointer");
bool sm_width_ok(int width) {
  for (int d = 1; d <= KSM_MAX_DIM; ++d)
    if ((width - d) % (2 * d) == 0 && ksm_ok((width - d) / (2 * d), d)) return true;
  return false;
}

// gram: the Gram-form kernels apply.  Column-count ladder (measured at n = 500 000, profiles/r02_s*_kv_small_t*.json):
//   1..4   kv_gramv (VALU contraction)            5..8   kv_gram4, two column groups of four (4x4x1 MFMA)
//   9..16  kv_gram16 (16-column 16x16x1_4B tile)  17..24 kv_gram4, six groups     25..  kv_gram (32-column tiles)
// flags (tuning / A-B only): GPAMD_KV_WIDE restores the older selection (VALU contraction up to 16 columns, the 32-column
// tile above), GPAMD_KV_G4 sends 9..12 columns to kv_gram4 with three groups
// small: few output rows (n < KGH_SMALL_N) -- the split kernels then take ONE 32-row tile per wave (128 rows per workgroup) so that
// the launch still spreads over the chip
// GPAMD_KV_BLOCK128 (the caller bounds the radius of 128-row blocks only): the split kernels take one row tile per wave (128 rows per workgroup, the
// `small` geometry), every other column count leaves the Gram form (its kernels centre 256 / 512-row blocks) for the direct-difference kernels
KvVariant pick_variant(int t, bool gram, int flags = 0, bool light = false, bool small = false, int dk = 16) {   // dk: kernel dims (light: dk <= 3 and RBF)  // t <= 129 handled per launch group; light: RBF, d <= 3
  KvVariant v{};
  const bool wide = flags & GPAMD_KV_WIDE;
  // GPAMD_KV_SPLIT_FEW: groups of fewer than five columns stay on the split-operand kernels too (a 32-column tile mostly empty: slower than the
  // few-column kernels when every tile is visited, faster when the caller culls far tiles -- only the split kernels walk tile lists)
  const int min_cols = (flags & GPAMD_KV_SPLIT_FEW) ? 1 : KGH_MIN_COLS;
  if (flags & GPAMD_KV_BLOCK128) {
    if (gram && (flags & GPAMD_KV_SPLIT) && t >= min_cols && t <= KGH_GROUP + 1) small = true;
    else gram = false;
  }
  v.gram = gram;
  if (gram && (flags & GPAMD_KV_SPLIT) && t >= min_cols && t <= KGH_GROUP + 1) {
    v.split = true;
    v.ex = (t % 32 == 1 && t > 1) ? 1 : 0;
    v.ct = (t - v.ex + 31) / 32;
    // four row tiles per wave with two column tiles ("lean", kv_gramh.hpp) where they fit: one Gram MFMA per block (dk <= 3) and, with the extra
    // column, the light generation of the RBF only (the other families would spill 7..15 registers there)
    v.ni = small ? 1 : kgh_ni(v.ct, (v.ex && !light && dk <= 16) ? 16 : dk);
    v.bm = kgh_bm(v.ni);
    v.bn = KGH_BN;
  } else if (!gram && (flags & GPAMD_KV_SPLIT) && t >= min_cols && t <= KDH_COLS + 1 && dk <= KDH_MAX_DIM) {
    // direct differences (clouds / rows outside the policy of the quadratic expansion, Matern nu = 1/2) with the contraction on the f16 matrix pipe
    // (kv_directh.hpp): the VALU keeps the generation only -- 9.8 instead of ~17 VALU instructions per pair at d = 3, eleven columns
    v.split = true;
    v.direct = true;
    v.ex = (t % 32 == 1 && t > 1) ? 1 : 0;
    v.ct = (t - v.ex + 31) / 32;
    v.ni = kdh_ni(small, v.ct, dk);
    v.bm = kdh_bm(v.ni);
    v.bn = KGH_BN;
  } else if (gram && !wide && t >= 5 && t <= 24 && dk <= 16) {   // (beyond 16 dimensions: no 4-column / 16-column tile kernels -- kv_gramv up to 16 columns, the 32-column tile above)
    if (t <= 8) v.g4 = 2;
    else if (t <= 12 && (flags & GPAMD_KV_G4)) v.g4 = 3;
    else if (t <= 16) v.g4 = 16;   // kv_gram16
    else if (t == 17) v.g4 = 17;   // kv_gram16 + the extra VALU column (16 probes + y)
    else v.g4 = 6;
    // RBF in <= 3 dimensions, 9..12 columns: generation is one v_exp_f32 per pair and three column groups on 4x4x1 beat the
    // 16-column tile by 7 % (64.0 vs 68.7 ms at n = 500 000, t = 11); every heavier generation (Matern: + v_sqrt_f32, d > 3:
    // more Gram MFMAs) does not issue under the 8-cycle MFMAs and is faster on the 16-column tile
    if (v.g4 == 16 && t <= 12 && light) v.g4 = 3;
    v.bm = v.g4 >= 16 ? KG16_BM : kg4_bm(v.g4);
    v.bn = v.g4 >= 16 ? KG16_BN : KG4_BN;
  } else if (t <= 8 || (gram && t <= 16) || (t <= 16 && dk <= 4)) {   // (direct differences, 9 .. 16 columns: kv_valu<T = 16> up to 4 dimensions -- 33 -> 27 ms per
    // product on the road3d shape (d = 3); at d = 10 the 32-column matrix-pipe tile wins, 0.83 against 1.16 ms on the protein shape's wide rows)
    v.valu = true;
    v.tpad = t <= 1 ? 1 : (t <= 2 ? 2 : (t <= 4 ? 4 : (t <= 8 ? 8 : 16)));
    v.bm = KVV_BM;
    v.bn = KVV_BN;
  } else {
    v.valu = false;
    if (t % 32 == 1 && t > 1) {
      v.ct = (t - 1) / 32;
      v.ex = 1;
    } else {
      v.ct = (t + 31) / 32;
      v.ex = 0;
    }
    v.bm = kv_bm_for_ct(v.ct, dk);
    v.bn = KV_BN;
  }
  return v;
}

constexpr int KV_GROUP = 128;  // columns per launch group (CT = 4); a trailing 129th column rides as EX

bool split_on(int kind, int flags) { return gram_ok(kind, flags) && (flags & GPAMD_KV_SPLIT); }

// split [0, t) into launch groups of <= cap (+1) columns: cap = 128, or 64 for the split-operand kernels
int group_cols(int t, int g0, int cap = KV_GROUP) { return (t - g0 <= cap + 1) ? t - g0 : cap; }   // (includes the cap + EX case)
bool prod_dims_ok(int d) { return d >= 2 && d <= 2 * KDP_MAX_FACTOR_DIM; }
static_assert(kv_kernel_dims(2 * KDP_MAX_FACTOR_DIM) == 2 * KDP_MAX_FACTOR_DIM, "every d the product family takes is an instantiated dimension (ptr_dims)");

// kernel of the product family for the code K_A + 4 K_B + 16 D_A and d = D_A + D_B; code < 0 (gpamd_kv_plan, which has no kparam): ANY instantiation of
// that d -- they share launch bounds and waves_per_eu, so the occupancy the plan asks for is the same
const void* prod_ptr(int code, int d, int ni, int ex) {
  static const Ptr4 kvp[4][4] = {{nullptr, kvp_kernel_ptr_rbf_m12, kvp_kernel_ptr_rbf_m32, kvp_kernel_ptr_rbf_m52},
                                 {nullptr, kvp_kernel_ptr_m12_m12, kvp_kernel_ptr_m12_m32, kvp_kernel_ptr_m12_m52},
                                 {nullptr, nullptr, kvp_kernel_ptr_m32_m32, kvp_kernel_ptr_m32_m52},
                                 {nullptr, nullptr, nullptr, kvp_kernel_ptr_m52_m52}};
  const ProdShape c = code < 0 ? ProdShape{GPAMD_RBF, GPAMD_MATERN12, d / 2} : prod_shape_of(code);
  const Ptr4 f = kvp[c.ka][c.kb];
  return f ? f(c.da, d - c.da, ni, ex) : nullptr;
}

// kernel of the additive family for the base family `code` and d; code < 0 (gpamd_kv_plan): ANY instantiation of that d -- the same launch bounds and waves_per_eu
const void* add_ptr(int code, int d, int ni, int ex) {
  typedef const void* (*Ptr3)(int, int, int);
  static const Ptr3 kva[4] = {kva_kernel_ptr_rbf, kva_kernel_ptr_matern12, kva_kernel_ptr_matern32, kva_kernel_ptr_matern52};
  if (code > 3) return nullptr;
  return kva[code < 0 ? 0 : code](d, ni, ex);
}

// kernel of the Newton-Girard additive family for code = base + 4 full and d; code < 0: ANY instantiation of that d -- the same launch bounds and
// waves_per_eu, which are those of the additive kernels too: the family is PLANNED as the additive family of the same d (gpamd_kv_plan does not take kind 9)
const void* ng_ptr(int code, int d, int ni, int ex) {
  static const Ptr4 kvn[4] = {kvn_kernel_ptr_rbf, kvn_kernel_ptr_matern12, kvn_kernel_ptr_matern32, kvn_kernel_ptr_matern52};
  if (code > 7) return nullptr;
  return code < 0 ? kvn[0](d, 0, ni, ex) : kvn[code & 3](d, code >> 2, ni, ex);
}

// kernel of the product-structure family for the base family `code` (1..3: Matern 1/2, 3/2, 5/2) and d; code < 0: ANY instantiation of that d -- the
// same launch bounds and waves_per_eu, which are those of the additive kernels too: PLANNED as the additive family of the same d, like the one above
const void* ps_ptr(int code, int d, int ni, int ex) {
  typedef const void* (*Ptr3)(int, int, int);
  static const Ptr3 kvt[4] = {nullptr, kvt_kernel_ptr_matern12, kvt_kernel_ptr_matern32, kvt_kernel_ptr_matern52};
  if (code > 3 || code == 0) return nullptr;
  return kvt[code < 0 ? 1 : code](d, ni, ex);
}

// kernel of the Gibbs family for the prepared width `width` (4, 8); it has no code: every parameter is in the rows
const void* gibbs_ptr(int, int width, int ni, int ex) { return kvg_kernel_ptr_gibbs(width, ni, ex); }

// kernel of the Hamming family for the prepared width `width` (4, 8, 16, 32 dwords); the same launch bounds and waves_per_eu as the Gibbs kernels and the same
// row-tile rule: PLANNED as the Gibbs family (gpamd_kv_plan does not take kind 12)
const void* ham_ptr(int, int width, int ni, int ex) { return kvham_kernel_ptr_packed(width, ni, ex); }
int ham_ni(bool small, int width) { return khm_ni(small, width); }
bool ham_width_ok(int width) { return khm_width_ok(width); }

// kernel of the spectral-mixture family for (Q, d) = (code >> 2, code & 3) and that prepared width; code < 0 (gpamd_kv_plan, which sees the width only): ANY
// instantiation of that width -- they share launch bounds and waves_per_eu
const void* sm_ptr(int code, int width, int ni, int ex) {
  int q = code >> 2, d = code & 3;
  if (code < 0) {
    for (d = 1; d <= KSM_MAX_DIM; ++d)
      if ((width - d) % (2 * d) == 0 && ksm_ok(q = (width - d) / (2 * d), d)) break;
  }
  if (!ksm_ok(q, d) || ksm_width(q, d) != width) return nullptr;
  if (d == 1) return q <= 4 ? kvsm_kernel_ptr_d1a(q, ni, ex) : kvsm_kernel_ptr_d1b(q, ni, ex);
  return d == 2 ? kvsm_kernel_ptr_d2(q, ni, ex) : kvsm_kernel_ptr_d3(q, ni, ex);
}

// The single-kernel families: ONE kernel each (direct differences + split contraction, any column count from 1 on; more than cols + 1 columns go in groups
// of `cols`, K regenerated per group), no Gram policy, no tile culling.  The caller says so with GPAMD_KV_SPLIT -- the flag that puts the f16 planes of V
// into the plan; without it the entry points refuse the family -- and every other flag is ignored: launches are planned and issued with family_flags, so
// pick_variant takes the direct-difference split branch with ct = 1 for every group.  A new such family is one row.
struct PrepTail { float coef_b; int da, nan_pad; };   // prep_points_kernel: the second factor's constant, the first factor's columns, NaN padding
struct OneKernelFamily {
  int kind;
  const char* name;               // "the <name> family ..." in the error messages
  int cols;                       // columns per launch group
  Ptr4 ptr;                       // kernel for (code, d, ni, ex), instantiated for every d the family takes; code < 0: any instantiation of that d
  int (*ni)(bool small, int d);   // own row-tile rule (nullptr: kdh_ni) -- a hook, not an exception in family_variant: such a family generates from the staged tile,
                                  // so the register rule of the direct-difference kernels (KDH_MAX_DIM) does not apply either: ONE dimension for the variant policy
  bool (*dims_ok)(int d); const char* takes;   // gpamd_kv_plan's envelope of d and what it says otherwise (nullptr: not planned under its own kind)
  bool kparam_code;               // kparam carries the family's code (kparam_error); else the code comes with its block
  bool own_entry;                 // the family travels with a device block: it comes through its own entry point, never through gpamd_kv_partials_f32
  PrepTail (*prep_tail)(int code, int dp);   // for gpamd_prep_points_f32 (nullptr: the plain tail)
};
const OneKernelFamily ONE_KERNEL[] = {
    {GPAMD_PROD, "product", KDP_COLS, prod_ptr, nullptr, prod_dims_ok, "takes d = D_A + D_B in 2..6", true, false,
     [](int code, int) { return PrepTail{prep_coef<float>(prod_shape_of(code).kb, 0.f), prod_shape_of(code).da, 0}; }},
    {GPAMD_SM, "spectral-mixture", KSM_COLS, sm_ptr, ksm_ni, sm_width_ok, "takes d = the prepared width D + 2 Q D, D in 1..3, Q <= 8 (D = 1) or 4", false, true, nullptr},
    // (instantiated for EVERY d in 2..8: a zero column is not neutral in a sum of covariances)
    {GPAMD_ADD, "additive", KDA_COLS, add_ptr, nullptr, kda_dims_ok, "takes d in 2..8", true, false, [](int, int dp) { return PrepTail{0.f, dp, 1}; }},
    // (planned as the additive family of the same d; known to its own entry point only: through every other one kind 9 stays the unknown kind it was)
    {GPAMD_NG, "Newton-Girard additive", KNG_COLS, ng_ptr, nullptr, kda_dims_ok, nullptr, false, true, nullptr},
    // (likewise: planned as the additive family of the same d, known to its own entry point only -- kind 11 stays unknown to every other one; it has no block,
    //  its entry point hands on the base family's id as the code)
    {GPAMD_PS, "product-structure", KPS_COLS, ps_ptr, nullptr, kda_dims_ok, nullptr, false, true, nullptr},
    // (known to its own entry point only -- kind 12 stays unknown to every other one; no block: 1 / alpha and beta ride by value (BlockLaunch::tail).  It
    //  generates from the staged tile like the spectral mixture, hence the own row-tile hook: ONE dimension for the variant policy, whatever the width)
    {GPAMD_HAMMING, "Hamming", KHM_COLS, ham_ptr, ham_ni, ham_width_ok, nullptr, false, true, nullptr},
    // (no code and no block: every parameter is in the prepared rows, whose width is its `d`; through gpamd_kv_plan / gpamd_kv_partials_f32 under its own kind)
    {GPAMD_GIBBS, "Gibbs", KGB_COLS, gibbs_ptr, nullptr, kgb_width_ok, "takes d = the prepared width 4 (up to two input dimensions) or 8 (up to six)", false, false, nullptr},
};
const OneKernelFamily* one_kernel(int kind) {
  for (const OneKernelFamily& f : ONE_KERNEL) if (f.kind == kind) return &f;
  return nullptr;
}
constexpr const char* SPLIT_ONLY = "runs on the split-contraction kernel only: pass GPAMD_KV_SPLIT";
int fail_family(const char* what, const OneKernelFamily* f, const char* rest) {   // "<what>: the <name> family <rest>"
  snprintf(g_err, sizeof(g_err), "%s: the %s family %s", what, f->name, rest);
  return GPAMD_EINVAL;
}
int policy_dims(int kind, int d) { const OneKernelFamily* f = one_kernel(kind); return (f && f->ni) ? 1 : d; }
// direct differences + split contraction (kv_directh.hpp): SPLIT without an applicable GRAM, up to KDH_MAX_DIM dimensions
bool dsplit_on(int kind, int flags, int d) { return !gram_ok(kind, flags) && (flags & GPAMD_KV_SPLIT) && kv_kernel_dims(policy_dims(kind, d)) <= KDH_MAX_DIM; }
int family_flags(int kind, int flags) { return one_kernel(kind) ? (GPAMD_KV_SPLIT | GPAMD_KV_SPLIT_FEW) : flags; }
int group_cap(int kind, int flags, int d) {
  const OneKernelFamily* f = one_kernel(kind);
  return f ? f->cols : (split_on(kind, flags) ? KGH_GROUP : (dsplit_on(kind, flags, d) ? KDH_COLS : KV_GROUP));
}
int ptr_dims(int kind, int d) { return one_kernel(kind) ? d : kv_kernel_dims(d); }   // what family_ptr takes as `d`
// ... and as `code`: the code that came with the family's block, or its kparam; -1 for every other family
int kernel_code(const OneKernelFamily* f, float kparam, const BlockLaunch* own) { return own ? own->code : ((f && f->kparam_code) ? (int)kparam : -1); }

// pick_variant for one launch group of `kind` (d: input dimensions; SM: prepared width)
KvVariant family_variant(int kind, int d, int t, int flags, bool small) {
  KvVariant v = pick_variant(t, gram_ok(kind, flags), flags, kind == GPAMD_RBF && d <= 3, small, kv_kernel_dims(policy_dims(kind, d)));
  const OneKernelFamily* f = one_kernel(kind);
  if (f && f->ni && v.direct) { v.ni = f->ni(small, d); v.bm = kdh_bm(v.ni); }
  return v;
}

// Split-operand launches keep, behind the S partial slabs of the workspace: column maxima | column multipliers | the two f16
// planes of every launch group (32 ct rows of ldh positions each).  Offsets in floats, all multiples of 4.
struct SplitLayout {
  int64_t base, colmax, colmul, planes, total;   // total: floats behind `base`
  int64_t ldh;
  int rows;                                      // plane rows over all split groups
};
SplitLayout split_layout(int kind, int flags, int m, int d, int t, int S, int64_t ldo) {
  SplitLayout L{};
  L.base = ((int64_t)S * t * ldo + 3) / 4 * 4;
  L.ldh = ((int64_t)m + KGH_BN - 1) / KGH_BN * KGH_BN;
  if (!split_on(kind, flags) && !dsplit_on(kind, flags, d)) return L;
  const int cap = group_cap(kind, flags, d);
  int rows = 0;
  for (int g0 = 0; g0 < t;) {
    const int tg = group_cols(t, g0, cap);
    KvVariant v = family_variant(kind, d, tg, flags, false);   // (row tiling does not change the plane rows)
    if (v.split) rows += 32 * v.ct;
    g0 += tg;
  }
  L.rows = rows;
  if (!rows) return L;
  const int64_t ncol = (2 * (int64_t)t + 64 + 3) / 4 * 4;   // 32 ct + 1 multiplier slots per group (<= t + 32 groups + 1)
  L.colmax = 0;
  L.colmul = ncol;
  L.planes = 2 * ncol;
  L.total = 2 * ncol + (int64_t)rows * L.ldh;    // two f16 planes = rows * ldh floats
  return L;
}

const void* family_ptr(int kind, int mode, int d, int v, int ex, int ni = 0, int code = -1) {
  if (const OneKernelFamily* f = one_kernel(kind)) return mode == KV_MODE_DIRECTH ? f->ptr(code, d, ni, ex) : nullptr;
  // one lookup per family and kernel group (kv_dispatch.hpp), indexed by the ABI's kind; no Gram-form kernels for Matern nu = 1/2
  static_assert(GPAMD_RBF == 0 && GPAMD_MATERN12 == 1 && GPAMD_MATERN32 == 2 && GPAMD_MATERN52 == 3 && GPAMD_RQ == 4 && GPAMD_PP == 5, "table order");
  typedef const void* (*Ptr2)(int, int);
  static const Ptr4 kvh[] = {kvh_kernel_ptr_rbf, nullptr, kvh_kernel_ptr_matern32, kvh_kernel_ptr_matern52, kvh_kernel_ptr_rq, kvh_kernel_ptr_pp};
  static const Ptr4 kvd[] = {kvd_kernel_ptr_rbf, kvd_kernel_ptr_matern12, kvd_kernel_ptr_matern32, kvd_kernel_ptr_matern52, kvd_kernel_ptr_rq, kvd_kernel_ptr_pp};
  static const Ptr2 kvm[] = {kvm_kernel_ptr_rbf, nullptr, kvm_kernel_ptr_matern32, kvm_kernel_ptr_matern52, kvm_kernel_ptr_rq, kvm_kernel_ptr_pp};
  static const Ptr2 kvs[] = {kvs_kernel_ptr_rbf, nullptr, kvs_kernel_ptr_matern32, kvs_kernel_ptr_matern52, kvs_kernel_ptr_rq, kvs_kernel_ptr_pp};
  static const Ptr4 kv[] = {kv_kernel_ptr_rbf, kv_kernel_ptr_matern12, kv_kernel_ptr_matern32, kv_kernel_ptr_matern52, kv_kernel_ptr_rq, kv_kernel_ptr_pp};
  if (kind < 0 || kind > GPAMD_PP) return nullptr;
  if (mode == KV_MODE_GRAMH) return kvh[kind] ? kvh[kind](d, v, ex, ni) : nullptr;
  if (mode == KV_MODE_DIRECTH) return kvd[kind](d, ni, v, ex);
  if (mode == KV_MODE_GRAM4) return kvm[kind] ? kvm[kind](d, v) : nullptr;
  if (mode == KV_MODE_GRAMV) return kvs[kind] ? kvs[kind](d, v) : nullptr;
  return kv[kind](mode, d, v, ex);
}

bool gram_ok(int kind, int flags) { return (flags & GPAMD_KV_GRAM) && kind != GPAMD_MATERN12; }

int kv_mode(int kind, int flags, int d, const KvVariant& v) {
  const bool gram = v.gram;   // (= gram_ok(kind, flags) unless GPAMD_KV_BLOCK128 sent this column group to the direct-difference kernels)
  if (v.split) return v.direct ? KV_MODE_DIRECTH : KV_MODE_GRAMH;
  if (v.g4) return KV_MODE_GRAM4;
  if (v.valu) return gram ? KV_MODE_GRAMV : KV_MODE_VALU;
  return gram ? KV_MODE_GRAM : KV_MODE_MFMA;
}

// tile geometry of the selected kernel (the small-t Gram variant uses its own row block / j tile)
void variant_geometry(int mode, KvVariant* v) {
  if (mode == KV_MODE_GRAMV) {
    v->bm = KGV_BM;
    v->bn = KGV_BN;
  }
}

int variant_key(const KvVariant& v) { return v.g4 ? v.g4 : (v.valu ? v.tpad : v.ct); }

// resident workgroups per CU of the selected kernel (runtime occupancy query; static table without a device)
int wg_per_cu(int kind, int mode, int dk, const KvVariant& v) {
  const void* fn = family_ptr(kind, mode, dk, variant_key(v), v.ex, v.ni);
  int nb = 0;
  if (fn && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, 0) == hipSuccess && nb > 0) return nb;
  (void)hipGetLastError();
  if (v.split) return 3;
  if (v.g4) return 2;
  if (v.valu) return 4;
  if (mode == KV_MODE_GRAM) return 3;
  return v.ct <= 2 ? 3 : 2;
}

void plan_split(int kind, int n, int m, int d, int t, int flags, int* S, int* jchunk) {
  // Grid = (row blocks) x (S chunks of the contracted index).  All units cost the same, so the launch
  // runs in ceil(units / slots) rounds of resident workgroups: pick the S whose last round is nearly
  // full (efficiency = units / (rounds * slots)), keeping every chunk >= 16 LDS tiles (per-unit prologue
  // and partial-slab write < 1 %) and preferring the smallest S among near-ties (less slab traffic).
  const int cap = group_cap(kind, flags, d);
  KvVariant v = family_variant(kind, d, group_cols(t, 0, cap), flags, n < KGH_SMALL_N);
  const int mode = kv_mode(kind, flags, d, v);
  variant_geometry(mode, &v);
  const int nrb = (n + v.bm - 1) / v.bm;
  const long slots = (long)num_cus() * wg_per_cu(kind, mode, ptr_dims(kind, d), v);
  const int min_chunk = 16 * v.bn;
  int smax = m / min_chunk;
  if (smax < 1) smax = (m >= 4 * v.bn) ? m / (4 * v.bn) : 1;  // small problems: favour parallelism
  // few output rows against many contracted ones (the wide-row launch of a block-centred product, a test set against the training set): 16-tile chunks
  // would leave most of the chip without a workgroup -- 72 workgroups for 9 000 x 36 584 pairs on the protein-shaped workload, 1.16 ms where the pairs
  // are worth 0.16 (profiles/r05_s4_workload_protein_kernel_stats.csv) -- so chunks go down to 4 tiles until one round of workgroups exists
  if ((long)nrb * smax < slots && m >= 8 * v.bn) {
    const long want = (slots + nrb - 1) / nrb;
    const int cap4 = m / (4 * v.bn);
    smax = (int)(want < cap4 ? want : cap4);
    if (smax < 1) smax = 1;
  }
  if (smax > 48) smax = 48;
  int best_s = 1;
  double best = -1.0;
  for (int s = 1; s <= smax; ++s) {
    const int jc = ((m + s - 1) / s + v.bn - 1) / v.bn * v.bn;
    const int se = (m + jc - 1) / jc;
    if (se != s) continue;  // rounding collapsed this split onto a smaller one
    const long units = (long)nrb * se;
    const long rounds = (units + slots - 1) / slots;
    // the last chunk is shorter than the others: count its units at their true relative cost
    const double last = (double)(m - (long)(se - 1) * jc) / (double)jc;
    const double work = (double)nrb * ((se - 1) + last);
    const double eff = work / ((double)rounds * (double)slots);
    if (eff > best + 0.01) {
      best = eff;
      best_s = s;
    }
  }
  const int jc = ((m + best_s - 1) / best_s + v.bn - 1) / v.bn * v.bn;
  *jchunk = jc;
  *S = (m + jc - 1) / jc;
}

}  // namespace

extern "C" {

int gpamd_abi_version(void) { return GPAMD_ABI_VERSION; }

const char* gpamd_last_error(void) { return g_err; }

int gpamd_prep_points_f32(int kind, float kparam, const float* X, int n, int d, int64_t ldx, const float* ls, int nls,
                          const float* shift, float* Xp, int dp, void* stream) {
  if (!kind_accepted(kind, KINDS_PREP)) return fail(GPAMD_EINVAL, "prep_points: unknown kind");
  if (const char* bad = kparam_error(kind, kparam, d)) return fail(GPAMD_EINVAL, "prep_points", bad);
  if (n <= 0 || d <= 0 || dp < d || dp % 4 || (nls != 1 && nls != d)) return fail(GPAMD_EINVAL, "prep_points: bad shape");
  if (!aligned16(Xp)) return fail(GPAMD_EINVAL, "prep_points: Xp must be 16-byte aligned");
  long total = (long)n * dp;
  unsigned grid = (unsigned)((total + 255) / 256);
  const OneKernelFamily* f = one_kernel(kind);
  const PrepTail tail = (f && f->prep_tail) ? f->prep_tail((int)kparam, dp) : PrepTail{0.f, dp, 0};
  hipLaunchKernelGGL(prep_points_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, n, d, ldx, ls, nls, shift,
                     prep_coef<float>(kind, kparam), Xp, dp, tail.coef_b, tail.da, tail.nan_pad);
  return check_launch("prep_points");
}

int gpamd_kv_plan(int kind, int n, int m, int d, int t, int flags, int64_t ldo, int* S_host, int* jchunk_host,
                  int64_t* workspace_floats_host) {
  if (!kind_accepted(kind, KINDS_KV) || n <= 0 || m <= 0 || t <= 0 || d < 1 || d > KV_MAX_DIM) return fail(GPAMD_EINVAL, "kv_plan: bad shape");
  const OneKernelFamily* f = one_kernel(kind);
  if (f && f->takes && !f->dims_ok(d)) return fail_family("kv_plan", f, f->takes);
  if (f && !(flags & GPAMD_KV_SPLIT)) return fail_family("kv_plan", f, SPLIT_ONLY);
  flags = family_flags(kind, flags);
  int S, jc;
  plan_split(kind, n, m, d, t, flags, &S, &jc);
  if (S_host) *S_host = S;
  if (jchunk_host) *jchunk_host = jc;
  if (workspace_floats_host) {
    const SplitLayout L = split_layout(kind, flags, m, d, t, S, ldo);
    *workspace_floats_host = L.total ? L.base + L.total : (int64_t)S * t * ldo;
  }
  return 0;
}

int gpamd_kv_partials_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt,
                          int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, int flags, const int* done,
                          void* stream) {
  return gpamd_kv_partials_far_f32(kind, kparam, X1p, n, X2p, m, d, X1c, Vt, ldv, t, P, ldo, S, jchunk, flags, done, stream, nullptr, nullptr, nullptr,
                                   nullptr, 0.f, nullptr, 0);
}

int64_t gpamd_kv_far_workspace_ints(int n, int S, int jchunk) {
  if (n <= 0 || S <= 0 || jchunk <= 0) return 0;
  return (int64_t)((n + 127) / 128) * S * (jchunk / 128 + 1);   // (the smallest row block of any kernel is 128 rows)
}

}  // extern "C"

namespace {
// gpamd_kv_partials_far_f32; with `own` the entry point of a family that travels with a block (spectral mixture: d = the prepared width; Newton-Girard; product structure; Hamming)
int kv_partials_impl(int kind, float kparam, const BlockLaunch* own, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt,
                     int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, int flags, const int* done, void* stream,
                     const float* row_centres, const float* row_radii, const float* tile_centres, const float* tile_radii, float sq_cutoff,
                     int* tile_ws, int64_t tile_ws_ints) {
  const OneKernelFamily* f = one_kernel(kind);   // (an own entry point names its family itself; of the block families KINDS_KV knows the spectral mixture only)
  if (!own && !kind_accepted(kind, KINDS_KV)) return fail(GPAMD_EINVAL, "kv: unknown kind");
  if (f && f->own_entry && !own) return fail(GPAMD_EINVAL, "kv: the spectral-mixture family travels with its parameter block (gpamd_kv_sm_partials_f32)");
  if (kind == GPAMD_PP || (f && f->kparam_code))
    if (const char* bad = kparam_error(kind, kparam, d)) return fail(GPAMD_EINVAL, "kv", bad);
  if (f && !own && f->takes && !f->dims_ok(d)) return fail_family("kv", f, f->takes);   // (a block family's own entry point has checked its shape)
  if (f && sq_cutoff > 0.f) return fail_family("kv", f, "is not culled (sq_cutoff must be 0)");
  if (f && !(flags & GPAMD_KV_SPLIT)) return fail_family("kv", f, SPLIT_ONLY);
  flags = family_flags(kind, flags);
  const bool cull = sq_cutoff > 0.f && row_centres && row_radii && tile_centres && tile_radii && tile_ws;
  if (sq_cutoff > 0.f && !cull) return fail(GPAMD_EINVAL, "kv: far-pair culling needs all four bounding-sphere arrays and the tile-list workspace");
  if (cull && (jchunk % 128 || S <= 0 || tile_ws_ints < gpamd_kv_far_workspace_ints(n, S, jchunk)))
    return fail(GPAMD_EINVAL, "kv: far-pair culling needs jchunk % 128 == 0 (gpamd_kv_plan) and gpamd_kv_far_workspace_ints(n, S, jchunk) ints of workspace");
  if (n <= 0 || m <= 0 || t <= 0 || S <= 0) return fail(GPAMD_EINVAL, "kv: bad shape");
  if (d < 1 || d > KV_MAX_DIM) return fail(GPAMD_EUNSUPPORTED, "kv: input dimension must be in 1..32");
  // kernels are instantiated for D in {1,2,3,4,5,6,8,10,12,16,20,24,32} valid dimensions; other d use the next one
  // (same padded stride, the extra coordinates are the zeros written by prep_points)
  const int dk = kv_kernel_dims(d);
  if (ldv % 4 || ldv < m || ldo < n) return fail(GPAMD_EINVAL, "kv: leading dimensions must be >= extent and ldv % 4 == 0");
  if (!aligned16(Vt) || !aligned16(X1p) || !aligned16(X2p) || !aligned16(X1c)) return fail(GPAMD_EINVAL, "kv: buffers must be 16-byte aligned");
  if (jchunk % 4 || (int64_t)jchunk * S < m) return fail(GPAMD_EINVAL, "kv: jchunk*S must cover m and jchunk % 4 == 0");
  hipStream_t st = (hipStream_t)stream;
  const int cap = group_cap(kind, flags, d);
  const SplitLayout L = split_layout(kind, flags, m, d, t, S, ldo);
  float* xbase = P + L.base;
  if (L.total) {
    if (!aligned16(P) || ldo % 4) return fail(GPAMD_EINVAL, "kv: the split-operand path needs a 16-byte aligned workspace and ldo % 4 == 0");
    if (jchunk % KGH_BN) return fail(GPAMD_EINVAL, "kv: the split-operand path needs jchunk % 128 == 0 (use gpamd_kv_plan)");
    (void)hipMemsetAsync(xbase + L.colmax, 0, sizeof(float) * (size_t)L.colmul, st);
  }
  int64_t prow = 0;   // plane rows used so far
  int mulslot = 0;    // multiplier slots used so far
  for (int g0 = 0; g0 < t;) {
    const int tg = group_cols(t, g0, cap);
    KvVariant v = family_variant(kind, d, tg, flags, n < KGH_SMALL_N);
    const int mode = kv_mode(kind, flags, d, v);
    variant_geometry(mode, &v);
    KvSmArgs ka;   // (KvhArgs + the block of the spectral-mixture or the Newton-Girard additive family, which only that family's kernels read)
    ka.sm = own ? own->block : nullptr;
    if (own && !own->block) memcpy(&ka.sm, own->tail, sizeof(own->tail));   // (a family without a block: its by-value parameters, zeros for the others)
    KvArgs& a = ka.a;
    a.X1 = X1p; a.X2 = X2p;
    a.Vt = Vt + (int64_t)g0 * ldv;
    a.P = P + (int64_t)g0 * ldo;
    a.ldv = ldv; a.ldo = ldo; a.pstride = (int64_t)t * ldo;
    a.n = n; a.m = m; a.t = tg;
    a.S = S; a.jchunk = jchunk;
    a.nrb = (n + v.bm - 1) / v.bm;
    a.done = done;
    a.kparam = kparam;
    a.Xc = X1c;
    if (cull && v.split) {
      // far-pair culling (split-operand kernels only, kv_mfma.hpp): this group's tile lists, built for ITS row block on the same stream
      const CullArgs c = cull_args(row_centres, row_radii, tile_centres, tile_radii, tile_ws, n, m, (dk + 3) / 4 * 4, v.bm, v.bn, a.nrb, jchunk, sq_cutoff, done);
      hipLaunchKernelGGL(cull_list_kernel<0>, dim3((unsigned)a.nrb * (unsigned)S), dim3(64), 0, st, c);
      a.tiles = tile_ws; a.tpc1 = c.tpc1;
    }
    unsigned grid = (unsigned)a.nrb * (unsigned)S;
    const void* fn = family_ptr(kind, mode, ptr_dims(kind, d), variant_key(v), v.ex, v.ni, kernel_code(f, kparam, own));
    if (!fn) return fail(GPAMD_EUNSUPPORTED, "kv: no kernel variant for this shape");
    if (v.split) {
      // pre-pass: per-column scale + the two f16 planes of this group's matrix-pipe columns (the extra column stays f32)
      const int tc = 32 * v.ct, tm = tg - v.ex;
      unsigned* colmax = reinterpret_cast<unsigned*>(xbase + L.colmax) + mulslot;
      float* colmul = xbase + L.colmul + mulslot;
      _Float16* vh = reinterpret_cast<_Float16*>(xbase + L.planes) + 2 * prow * L.ldh;
      _Float16* vl = vh + (int64_t)tc * L.ldh;
      unsigned nbm = (unsigned)((m + 4095) / 4096);
      if (nbm > 64) nbm = 64;
      hipLaunchKernelGGL(vsplit_colmax_kernel, dim3(nbm, tm), dim3(256), 0, st, a.Vt, ldv, m, colmax, done);
      hipLaunchKernelGGL(vsplit_kernel, dim3((unsigned)((L.ldh / 8 + 255) / 256), tc), dim3(256), 0, st, a.Vt, ldv, m, tm, vh, vl,
                         L.ldh, (const unsigned*)colmax, colmul, done);
      ka.Vh = vh; ka.Vl = vl; ka.ldh = L.ldh; ka.colmul = colmul;
      prow += tc;
      mulslot += tc + 1;
      void* kargs[] = {(void*)&ka};
      (void)hipLaunchKernel(fn, dim3(grid), dim3(256), kargs, 0, st);
    } else {
      void* kargs[] = {(void*)&a};
      (void)hipLaunchKernel(fn, dim3(grid), dim3(256), kargs, 0, st);
    }
    int rc = check_launch("kv_partials");
    if (rc) return rc;
    g0 += tg;
  }
  return 0;
}
}  // namespace

extern "C" {

int gpamd_kv_partials_far_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt,
                              int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, int flags, const int* done, void* stream,
                              const float* row_centres, const float* row_radii, const float* tile_centres, const float* tile_radii, float sq_cutoff,
                              int* tile_ws, int64_t tile_ws_ints) {
  return kv_partials_impl(kind, kparam, nullptr, X1p, n, X2p, m, d, X1c, Vt, ldv, t, P, ldo, S, jchunk, flags, done, stream, row_centres, row_radii,
                          tile_centres, tile_radii, sq_cutoff, tile_ws, tile_ws_ints);
}

int gpamd_kv_sm_partials_f32(const float* block, int q, int d, const float* X1p, int n, const float* X2p, int m, int width, const float* Vt, int64_t ldv,
                             int t, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (!ksm_ok(q, d)) return fail(GPAMD_EUNSUPPORTED, "kv_sm: (Q, d) outside the native envelope: d in 1..3, Q in 1..8 (d = 1) or 1..4 (d = 2, 3)");
  if (!block) return fail(GPAMD_EINVAL, "kv_sm: null parameter block");
  if (width != ksm_width(q, d)) return fail(GPAMD_EINVAL, "kv_sm: the prepared width must be d + 2 Q d");
  const BlockLaunch own{block, 4 * q + d};
  return kv_partials_impl(GPAMD_SM, 0.f, &own, X1p, n, X2p, m, width, nullptr, Vt, ldv, t, P, ldo, S, jchunk, GPAMD_KV_SPLIT, done, stream, nullptr, nullptr,
                          nullptr, nullptr, 0.f, nullptr, 0);
}

int gpamd_kv_ng_partials_f32(const float* block, int base, int d, int max_degree, const float* X1p, int n, const float* X2p, int m, const float* Vt,
                             int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (!kda_dims_ok(d)) return fail(GPAMD_EUNSUPPORTED, "kv_ng: d outside the native envelope 2..8");
  if (!block) return fail(GPAMD_EINVAL, "kv_ng: null weight block");
  if (base < 0 || base > 3) return fail(GPAMD_EINVAL, "kv_ng: base must be the base family's id: 0 (RBF), 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!kng_ok(d, max_degree)) return fail(GPAMD_EINVAL, "kv_ng: max_degree must be in 1..d");
  const BlockLaunch own{block, base + 4 * (ng_cap(d, max_degree) == d ? 1 : 0)};
  return kv_partials_impl(GPAMD_NG, 0.f, &own, X1p, n, X2p, m, d, nullptr, Vt, ldv, t, P, ldo, S, jchunk, GPAMD_KV_SPLIT, done, stream, nullptr, nullptr,
                          nullptr, nullptr, 0.f, nullptr, 0);
}

int gpamd_kv_ps_partials_f32(int base, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P, int64_t ldo,
                             int S, int jchunk, const int* done, void* stream) {
  if (!kda_dims_ok(d)) return fail(GPAMD_EUNSUPPORTED, "kv_ps: d outside the native envelope 2..8");
  if (base == GPAMD_RBF) return fail(GPAMD_EINVAL, "kv_ps: a product of one-dimensional RBFs IS the RBF family with per-dimension lengthscales (GPAMD_RBF): base must be 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  if (!kps_base_ok(base)) return fail(GPAMD_EINVAL, "kv_ps: base must be the base family's id: 1, 2 or 3 (Matern 1/2, 3/2, 5/2)");
  const BlockLaunch own{nullptr, base};   // (no block: base family and d are template arguments of the kernel)
  return kv_partials_impl(GPAMD_PS, 0.f, &own, X1p, n, X2p, m, d, nullptr, Vt, ldv, t, P, ldo, S, jchunk, GPAMD_KV_SPLIT, done, stream, nullptr, nullptr,
                          nullptr, nullptr, 0.f, nullptr, 0);
}

int gpamd_kv_hamming_partials_f32(int width, float inv_alpha, float beta, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                  float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  if (!khm_width_ok(width)) return fail(GPAMD_EUNSUPPORTED, "kv_hamming: the prepared width must be 4, 8, 16 or 32 dwords (up to 16, 32, 64, 128 positions)");
  if (!khm_param_ok(inv_alpha) || !khm_param_ok(beta)) return fail(GPAMD_EINVAL, "kv_hamming: 1 / alpha and beta must be positive and finite");
  BlockLaunch own{nullptr, width};   // (no block: the width is a template argument of the kernel, the two parameters ride by value)
  own.tail[0] = inv_alpha; own.tail[1] = beta;
  return kv_partials_impl(GPAMD_HAMMING, 0.f, &own, X1p, n, X2p, m, width, nullptr, Vt, ldv, t, P, ldo, S, jchunk, GPAMD_KV_SPLIT, done, stream, nullptr, nullptr,
                          nullptr, nullptr, 0.f, nullptr, 0);
}

int gpamd_kv_reduce_f32(const float* P, int S, int64_t ldp, int t, int n, const float* scale, const float* dscale,
                        const float* dvec, const float* Vd, int64_t ldd, float* Out, int64_t ldo, const int* done,
                        void* stream) {
  if (S <= 0 || t <= 0 || n <= 0) return fail(GPAMD_EINVAL, "kv_reduce: bad shape");
  if (ldp % 4 || ldo % 4 || (Vd && ldd % 4)) return fail(GPAMD_EINVAL, "kv_reduce: leading dimensions must be multiples of 4");
  dim3 grid(col_blocks(n, CG_MAXNB), t);
  hipLaunchKernelGGL((kv_reduce_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, P, S, (int64_t)t * ldp, ldp,
                     scale, dscale, dvec, Vd, ldd, Out, ldo, n, (float*)nullptr, done);
  return check_launch("kv_reduce");
}

int gpamd_kv_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt, int64_t ldv,
                 int t, const float* scale, const float* dscale, const float* Vd, int64_t ldd, float* Out,
                 int64_t ldo, float* workspace, int64_t workspace_floats, int flags, void* stream) {
  int S, jc;
  if (!kind_accepted(kind, KINDS_PREP) || n <= 0 || m <= 0 || t <= 0 || d < 1 || d > KV_MAX_DIM) return fail(GPAMD_EINVAL, "kv: bad shape");
  const OneKernelFamily* f = one_kernel(kind);
  if (f && f->kparam_code)
    if (const char* bad = kparam_error(kind, kparam, d)) return fail(GPAMD_EINVAL, "kv", bad);
  if (f && !(flags & GPAMD_KV_SPLIT)) return fail_family("kv", f, SPLIT_ONLY);
  flags = family_flags(kind, flags);
  plan_split(kind, n, m, d, t, flags, &S, &jc);
  const int64_t ldp = (n + 3) / 4 * 4;
  const SplitLayout L = split_layout(kind, flags, m, d, t, S, ldp);
  if (workspace_floats < (L.total ? L.base + L.total : (int64_t)S * t * ldp))
    return fail(GPAMD_EWORKSPACE, "kv: workspace too small (use gpamd_kv_plan with ldo = round_up(n,4) and the same flags)");
  int rc = gpamd_kv_partials_f32(kind, kparam, X1p, n, X2p, m, d, X1c, Vt, ldv, t, workspace, ldp, S, jc, flags, nullptr, stream);
  if (rc) return rc;
  return gpamd_kv_reduce_f32(workspace, S, ldp, t, n, scale, dscale, nullptr, Vd, ldd, Out, ldo, nullptr, stream);
}

int gpamd_kernel_rows_f32(int kind, float kparam, const float* X1p, const int64_t* rows, int nrows, const float* X2p, int m, int dp,
                          const float* scale, float* out, int64_t ldo, void* stream) {
  if (nrows <= 0 || m <= 0 || dp <= 0 || ldo < m) return fail(GPAMD_EINVAL, "kernel_rows: bad shape (nrows, m, dp >= 1; ldo >= m)");
  if (nrows > 65535) return fail(GPAMD_EUNSUPPORTED, "kernel_rows: nrows > 65535 (call it in blocks of 65535 rows)");
  dim3 grid((m + 255) / 256, nrows);
  if (const char* bad = pointwise_error(kind, kparam, dp)) return fail(GPAMD_EINVAL, "kernel_rows", bad);
  if (!with_kind<KINDS_POINTWISE>(kind, [&](auto K) {
        hipLaunchKernelGGL((kernel_rows_kernel<K()>), grid, dim3(256), 0, (hipStream_t)stream, X1p, rows, nrows, X2p, m, dp, scale, out, ldo, kparam);
      }))
    return fail(GPAMD_EINVAL, "unknown kind");
  return check_launch("kernel_rows");
}

int gpamd_kernel_dense_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int dp, const float* scale,
                           float* out, int64_t ldo, void* stream) {
  if (n <= 0 || m <= 0 || dp <= 0 || ldo < m) return fail(GPAMD_EINVAL, "kernel_dense: bad shape (n, m, dp >= 1; ldo >= m)");
  if (n > 65535) return fail(GPAMD_EUNSUPPORTED, "kernel_dense: n > 65535 (materialising K is what this library avoids)");
  dim3 grid((m + 255) / 256, n);
  if (const char* bad = pointwise_error(kind, kparam, dp)) return fail(GPAMD_EINVAL, "kernel_dense", bad);
  if (!with_kind<KINDS_POINTWISE>(kind, [&](auto K) {
        hipLaunchKernelGGL((kernel_dense_kernel<K()>), grid, dim3(256), 0, (hipStream_t)stream, X1p, n, X2p, m, dp, scale, out, ldo, kparam);
      }))
    return fail(GPAMD_EINVAL, "unknown kind");
  return check_launch("kernel_dense");
}

int gpamd_kernel_diag_f32(int kind, float kparam, const float* X1p, const float* X2p, int n, int dp, const float* scale, float* out,
                          void* stream) {
  if (n <= 0) return fail(GPAMD_EINVAL, "kernel_diag: bad shape");
  dim3 grid((n + 255) / 256);
  if (const char* bad = pointwise_error(kind, kparam, dp)) return fail(GPAMD_EINVAL, "kernel_diag", bad);
  if (!with_kind<KINDS_POINTWISE>(kind, [&](auto K) {
        hipLaunchKernelGGL((kernel_diag_kernel<K()>), grid, dim3(256), 0, (hipStream_t)stream, X1p, X2p, n, dp, scale, out, kparam);
      }))
    return fail(GPAMD_EINVAL, "unknown kind");
  return check_launch("kernel_diag");
}

int gpamd_coldot_f32(const float* A, const float* B, int64_t ld, int n, int t, float* out, float* scratch,
                     void* stream) {
  if (n <= 0 || t <= 0 || ld % 4) return fail(GPAMD_EINVAL, "coldot: bad shape");
  unsigned nb = col_blocks(n, CG_MAXNB);
  hipLaunchKernelGGL((coldot_kernel<float>), dim3(nb, t), dim3(256), 0, (hipStream_t)stream, A, B, ld, n, scratch,
                     (const int*)nullptr);
  hipLaunchKernelGGL((colsum_partials_kernel<float>), dim3(t), dim3(256), 0, (hipStream_t)stream, scratch, (int)nb, out);
  return check_launch("coldot");
}

// ------------------------------------------------------------------------------------------- mBCG
struct gpamd_cg : CgHandle<float> {};

int64_t gpamd_cg_fscratch_elems(int t, int hist_len) { return cg_scratch(t, hist_len).total; }
int64_t gpamd_cg_iscratch_elems(int t) { return (int64_t)2 * t + 2; }

int gpamd_cg_layout(int t, int hist_len, int64_t* o) {
  if (!o) return fail(GPAMD_EINVAL, "cg_layout: null output");
  const CgScratch L = cg_scratch(t, hist_len);
  o[0] = L.bnorm; o[1] = L.rnorm; o[2] = L.alpha_hist; o[3] = L.beta_hist; o[4] = L.stats;
  return 0;
}

// row-sharded solves: the host all-reduces these partial sums between the *_norms / *_apply and dot_rz / *_apply steps
int gpamd_cg_partials_layout(int n, int t, int hist_len, int64_t* offs, int* stride, int* nb) {
  if (!offs || !stride || !nb || n <= 0 || t <= 0 || hist_len < 0) return fail(GPAMD_EINVAL, "cg_partials_layout: bad arguments");
  const CgScratch L = cg_scratch(t, hist_len);
  offs[0] = L.part_a; offs[1] = L.part_rz; offs[2] = L.part_rr;
  *stride = CG_MAXNB;
  *nb = (int)col_blocks(n, CG_MAXNB);
  return 0;
}

gpamd_cg_t* gpamd_cg_create_f32(int n, int t, int64_t ld, float* X, float* R, float* D, float* Q, float* Z,
                                float* fscratch, int* iscratch, int hist_len, float eps, float stop_updating_after) {
  gpamd_cg h;
  return cg_setup("cg_create", h.st, n, t, ld, X, R, D, Q, Z, fscratch, iscratch, hist_len, eps, stop_updating_after) ? new gpamd_cg(h) : nullptr;
}
void gpamd_cg_destroy(gpamd_cg_t* h) { delete h; }
const int* gpamd_cg_done_ptr(const gpamd_cg_t* h) { return h ? h->st.done : nullptr; }

int gpamd_cg_init_f32(gpamd_cg_t* h, const float* B, int64_t ldb, int have_precond, void* stream) { return cg_init("cg_init", h, B, ldb, have_precond, stream); }
int gpamd_cg_init_norms_f32(gpamd_cg_t* h, const float* B, int64_t ldb, void* stream) { return cg_init_norms("cg_init_norms", h, B, ldb, stream); }
int gpamd_cg_init_apply_f32(gpamd_cg_t* h, const float* B, int64_t ldb, int copy_d, void* stream) { return cg_init_apply("cg_init_apply", h, B, ldb, copy_d, stream); }
int gpamd_cg_begin_apply_f32(gpamd_cg_t* h, void* stream) { return cg_begin_apply("cg_begin_apply", h, stream); }
int gpamd_cg_dot_rz_f32(gpamd_cg_t* h, void* stream) { return cg_dot_rz("cg_dot_rz", h, stream); }
int gpamd_cg_update_d_apply_f32(gpamd_cg_t* h, int k, void* stream) { return cg_update_d_apply("cg_update_d_apply", h, k, stream); }
int gpamd_cg_begin_f32(gpamd_cg_t* h, void* stream) { return cg_begin("cg_begin", h, stream); }
int gpamd_cg_reduce_q_f32(gpamd_cg_t* h, const float* P, int S, int64_t ldp, const float* scale, const float* dscale,
                          const float* dvec, void* stream) {
  return cg_reduce_q("cg_reduce_q", h, P, S, ldp, scale, dscale, dvec, stream);
}
int gpamd_cg_update_xr_f32(gpamd_cg_t* h, int k, void* stream) { return cg_update_xr("cg_update_xr", h, k, stream); }
int gpamd_cg_update_d_f32(gpamd_cg_t* h, int k, void* stream) { return cg_update_d("cg_update_d", h, k, stream); }
int gpamd_cg_stop_f32(gpamd_cg_t* h, int k, int min_iter, int tridiag_floor, float tol, void* stream) {
  return cg_stop("cg_stop", h, k, min_iter, tridiag_floor, tol, stream);
}
int gpamd_cg_finish_f32(gpamd_cg_t* h, void* stream) { return cg_finish("cg_finish", h, stream); }

// ----------------------------------------------------------------------------- pivoted Cholesky
int gpamd_pivoted_cholesky_f32(int kind, float kparam, const float* Xp, int n, int dp, const float* scale, int rank, float tol,
                               float* L, int64_t ldl, int64_t* pivots, float* fwork, int* iwork, void* stream) {
  if (n <= 0 || rank <= 0 || ldl < n) return fail(GPAMD_EINVAL, "pivoted_cholesky: bad shape");
  if (rank > PC_MAX_RANK) return fail(GPAMD_EUNSUPPORTED, "pivoted_cholesky: rank > 512");
  if (const char* bad = pointwise_error(kind, kparam, dp)) return fail(GPAMD_EINVAL, "pivoted_cholesky", bad);
  if (rank > n) rank = n;
  hipStream_t st = (hipStream_t)stream;
  PcState s;
  s.dwork = fwork;
  s.scal = fwork + n;
  s.L = L; s.ldl = ldl; s.n = n; s.rank = rank;
  s.pivots = pivots;
  s.ctl = iwork;
  s.perm = iwork + 2;
  s.pos = iwork + 2 + n;
  s.tol = tol;
  s.kparam = kparam;
  (void)hipMemsetAsync(iwork, 0, 2 * sizeof(int), st);
  const int nb = (n + 255) / 256;
  if (n >= 8) {
    // one launch per pivot step: the update of step m and the arg-max for step m + 1 in one kernel (misc_kernels.hpp, "last block decides");
    // the partials live in the former permutation region of iwork (4 nb + 1 <= n words for n >= 8)
    PcPartials pp;
    pp.nb = nb;
    pp.ppos = s.perm;
    pp.pidx = s.perm + nb;
    pp.pval = reinterpret_cast<float*>(s.perm + 2 * nb);
    pp.psum = reinterpret_cast<float*>(s.perm + 3 * nb);
    pp.counter = reinterpret_cast<unsigned*>(s.perm + 4 * nb);
    (void)hipMemsetAsync(pp.counter, 0, sizeof(unsigned), st);
    if (!with_kind<KINDS_POINTWISE>(kind, [&](auto K) { hipLaunchKernelGGL((pc_first_kernel<K()>), dim3(nb), dim3(256), 0, st, s, pp, Xp, dp, scale); }))
      return fail(GPAMD_EINVAL, "unknown kind");
    for (int m = 0; m < rank; ++m)
      with_kind<KINDS_POINTWISE>(kind, [&](auto K) { hipLaunchKernelGGL((pc_step_kernel<K()>), dim3(nb), dim3(256), 0, st, s, pp, m, Xp, dp, scale); });
    return check_launch("pivoted_cholesky");
  }
  hipLaunchKernelGGL(pc_init_perm_kernel, dim3(nb), dim3(256), 0, st, s.perm, s.pos, n);
  // diagonal of the noise-free kernel matrix: scale * k(0)
  if (!with_kind<KINDS_POINTWISE>(kind, [&](auto K) { hipLaunchKernelGGL((kernel_diag_kernel<K()>), dim3(nb), dim3(256), 0, st, Xp, Xp, n, dp, scale, s.dwork, kparam); }))
    return fail(GPAMD_EINVAL, "unknown kind");
  for (int m = 0; m < rank; ++m) {
    hipLaunchKernelGGL(pc_pivot_kernel, dim3(1), dim3(1024), 0, st, s, m);
    with_kind<KINDS_POINTWISE>(kind, [&](auto K) { hipLaunchKernelGGL((pc_update_kernel<K()>), dim3(nb), dim3(256), 0, st, s, m, Xp, dp, scale); });
  }
  return check_launch("pivoted_cholesky");
}

// ----------------------------------------------------------------------------- RCCL-communicator variants (multi-GPU hosts without torch)
// librccl is resolved lazily (dlopen / dlsym) so that the library keeps loading on single-GPU hosts without it.
namespace {
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
nccl_allreduce_fn rccl_allreduce() {
  // function-local static with a lambda initialiser: initialised exactly once, thread-safe by the language rules (no "tried" flag that a
  // second thread could observe set while the pointer is still null)
  static const nccl_allreduce_fn fn = []() -> nccl_allreduce_fn {
    void* hdl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!hdl) hdl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    return hdl ? reinterpret_cast<nccl_allreduce_fn>(dlsym(hdl, "ncclAllReduce")) : nullptr;
  }();
  return fn;
}
}  // namespace

int gpamd_allreduce_sum_f32(float* buf, int64_t count, void* rccl_comm, void* stream) {
  if (!buf || count <= 0 || !rccl_comm) return fail(GPAMD_EINVAL, "allreduce_sum: bad arguments");
  nccl_allreduce_fn fn = rccl_allreduce();
  if (!fn) return fail(GPAMD_EUNSUPPORTED, "allreduce_sum: librccl.so (ncclAllReduce) not found");
  const int rc = fn(buf, buf, (size_t)count, /*ncclFloat32*/ 7, /*ncclSum*/ 0, rccl_comm, (hipStream_t)stream);
  if (rc != 0) return fail(GPAMD_EINVAL, "allreduce_sum: ncclAllReduce failed");
  return 0;
}

int gpamd_cg_stop_comm_f32(gpamd_cg_t* h, int k, int min_iter, int tridiag_floor, float tol, void* rccl_comm, void* stream) {
  if (!h) return fail(GPAMD_EINVAL, "cg_stop_comm: null handle");
  if (rccl_comm) {
    const int rc = gpamd_allreduce_sum_f32(h->st.stats, 2, rccl_comm, stream);
    if (rc) return rc;
  }
  return gpamd_cg_stop_f32(h, k, min_iter, tridiag_floor, tol, stream);
}

}  // extern "C"
