/* gpamd.h -- C ABI of the MI355X-native BBMM hot path (libgpamd.so, gfx950 only).
 *
 * The reference (cornellius-gp/gpytorch + the third-party linear_operator package) has NO native
 * boundary: its hot path is Python calling torch.  These entry points are what a ctypes / cffi /
 * torch-extension binding for that path binds instead; each one cites the reference interface it
 * replaces.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; no ownership transfer;
 *   - `stream` is a hipStream_t (NULL = default stream); all calls are asynchronous on it;
 *   - return value: 0 on success, a positive hipError_t, or a negative GPAMD_E* argument error;
 *     gpamd_last_error() returns a thread-local message for the last non-zero return;
 *   - vectors are "probe-major": a block of t right-hand sides is float[t][ld], ld >= n, ld % 4 == 0,
 *     base 16-byte aligned (row c = probe c, contiguous over the n data points);
 *   - point clouds are first converted by gpamd_prep_points_f32 into float[n][dp], dp = 4*ceil(d/4),
 *     pre-scaled so that every kernel evaluates k = f(|zi - zj|^2) only.
 */
#ifndef GPAMD_H
#define GPAMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPAMD_ABI_VERSION 5

/* covariance families: gpytorch/kernels/rbf_kernel.py:68-85, matern_kernel.py:85-110 (nu = 1/2, 3/2, 5/2) */
enum { GPAMD_RBF = 0, GPAMD_MATERN12 = 1, GPAMD_MATERN32 = 2, GPAMD_MATERN52 = 3,
       GPAMD_RQ = 4 /* rational quadratic (gpytorch/kernels/rq_kernel.py:60-74): k = (1 + |z - z'|^2)^-alpha on points prepared as
                       x / (l sqrt(2 alpha)); float32 and float64, any input dimension */,
       GPAMD_PP = 5 /* piecewise polynomial with compact support (gpytorch/kernels/piecewise_polynomial_kernel.py:11-28, 104-121):
                       k = max(1 - r, 0)^(j+q) P_q(r), r = |z - z'| on points prepared as x / l, EXACTLY zero from r = 1 on.  `kparam` carries the two
                       integers as the code 4 j + q (q in 0..3, j >= q + 1; the reference sets j = floor(D / 2) + q + 1); any other value is
                       GPAMD_EINVAL.  P_2's r^2 coefficient is the one the reference's code evaluates, (j + 4 j + 3) / 3 -- not the (j^2 + 4 j + 3) / 3
                       of its docstring.  q = 0 has a cusp at r = 0 like Matern nu = 1/2: callers keep it off GPAMD_KV_GRAM and off
                       gpamd_kv_grad2_f32 (which refuses it; gpamd_kv_grad_param_far_f32 serves it).  Additive: the ABI version stays 5.  Far-pair culling with sq_cutoff = 1 is exact. */,
       GPAMD_PROD = 6 /* product of two parameter-free stationary factors over two column groups of the prepared cloud (gpytorch/kernels/kernel.py:634-688
                       restricted to two members): k = k_A(|z_A - z_A'|) k_B(|z_B - z_B'|), A, B in {RBF, Matern 1/2, 3/2, 5/2} by their GPAMD_* ids.
                       `kparam` carries the code K_A + 4 K_B + 16 D_A and `d` = D_A + D_B: the prepared row is [z_A | z_B | zeros] with stride
                       round_up(d, 4); gpamd_prep_points_f32 scales the first D_A columns by the factor of family K_A and the others by that of K_B.
                       Canonical order, anything else is GPAMD_EINVAL: an integer code, K_A <= K_B <= 3, not both RBF (that product is one RBF), 1 <= D_A <= 3,
                       1 <= d - D_A <= 3, and D_A <= d - D_A where K_A = K_B.  float32 only, ONE product kernel (direct differences + split contraction,
                       kv_directp.hpp): gpamd_kv_plan / gpamd_kv_partials_f32 / gpamd_kv_f32 take the family with GPAMD_KV_SPLIT only (GPAMD_EINVAL without it) and ignore every other flag (the plan always
                       holds the f16 planes of V; more than 33 columns go in groups of 32), sq_cutoff must be 0.  Accepted by gpamd_prep_points_f32,
                       gpamd_kv_plan, gpamd_kv_partials_f32, gpamd_kv_f32, gpamd_kernel_rows_f32, gpamd_kernel_dense_f32, gpamd_kernel_diag_f32,
                       gpamd_pivoted_cholesky_f32 and gpamd_kv_grad_param_far_f32 (per-dimension sums: iso must be 0; sq_cutoff 0); every other entry
                       point refuses it.  Additive: the ABI version stays 5. */,
       GPAMD_SM = 7 /* spectral mixture as the reference executes it (gpytorch/kernels/spectral_mixture_kernel.py:336-352: the sum over the Q mixtures
                       before the product over the d dimensions): k = Wsum^d k~, k~ = prod_j sum_q w^_q exp(-2 pi^2 sigma_qj^2 tau_j^2) cos(2 pi mu_qj tau_j),
                       tau = x - x', w^ = w / Wsum, Wsum = sum_q w_q.  The library evaluates k~ in [-1, 1]; the caller applies Wsum^d as the `scale` of
                       gpamd_kv_reduce_f32.  The prepared row (the caller's arithmetic: phases reduced to [0, 1) in float64 BEFORE cos / sin and the cast) is
                       [x - shift (d) | sqrt(w^_q) cos(2 pi frac(x_j mu_qj)), sqrt(w^_q) sin(...) at columns d + 2 (q d + j), + 1 | zeros], width d + 2 Q d,
                       stride round_up(width, 4); the parameter block is Q d device floats na[q d + j] = -2 pi^2 sigma_qj^2 log2(e).  Native envelope:
                       float32, d in 1..3, Q in 1..8 (d = 1) or 1..4 (d = 2, 3).  Entry points: gpamd_kv_plan (kind = GPAMD_SM, `d` = the prepared WIDTH,
                       GPAMD_KV_SPLIT required), gpamd_kv_sm_partials_f32, gpamd_kv_sm_grad_f32 (+ its workspace query); every other entry point that
                       takes a `kind` refuses it -- rows, dense blocks and diagonals of this family are the caller's (backend.sm_dense).  Never culled.
                       Additive: the ABI version stays 5. */,
       GPAMD_ADD = 8 /* first-order additive structure over a parameter-free one-dimensional base family (gpytorch/kernels/additive_structure_kernel.py:62-68,
                       which sums a d x n x m tensor): k = d k~, k~ = (1/d) sum_{q<d} k'(|z_q - z_q'|), k' in {RBF, Matern 1/2, 3/2, 5/2}.  The library
                       evaluates the MEAN k~ -- unit diagonal, values in [0, 1] like every other family --; the caller's `scale` carries d x outputscale.
                       `kparam` carries the base family's id 0..3, any other value is GPAMD_EINVAL; `d` is 2..8.  gpamd_prep_points_f32 prepares the rows
                       as the base family prescribes (one lengthscale or d, stride round_up(d, 4)) and writes NaN -- not zero -- into the padding columns:
                       a zero column would count as one more dimension with k'(0) = 1, and the entry points that see the padded stride only count d from
                       them.  float32 only, ONE product kernel (kv_directadd.hpp: d one-dimensional covariances per pair summed in registers, one split
                       contraction): gpamd_kv_plan / gpamd_kv_partials_f32 / gpamd_kv_f32 take the family with GPAMD_KV_SPLIT only (GPAMD_EINVAL without it)
                       and ignore every other flag (the plan always holds the f16 planes of V; more than 33 columns go in groups of 32), sq_cutoff must
                       be 0.  Accepted by exactly the entry points that accept GPAMD_PROD -- gpamd_prep_points_f32, gpamd_kv_plan, gpamd_kv_partials_f32,
                       gpamd_kv_f32, gpamd_kernel_rows_f32, gpamd_kernel_dense_f32, gpamd_kernel_diag_f32, gpamd_pivoted_cholesky_f32 and
                       gpamd_kv_grad_param_far_f32 (per-dimension sums G[1 + q] = sum W (1/d) dk'/ds(s_q) s_q, s_q = (z_q - z_q')^2: iso must be 0;
                       sq_cutoff 0) --; every other entry point refuses it.  Additive: the ABI version stays 5. */,
       GPAMD_NG = 9 /* additive structure WITH interactions over a parameter-free one-dimensional base family -- Duvenaud's additive GP, the reference's
                       NewtonGirardAdditiveKernel (gpytorch/kernels/newton_girard_additive_kernel.py, which forms a d x n x m tensor, R power sums of it and
                       R + 1 polynomials): k = sum_{n=1..R} sigma_n e_n(z_1 .. z_d), z_q = k'(|x_q - x_q'|), k' in {RBF, Matern 1/2, 3/2, 5/2}, e_n the n-th
                       elementary symmetric polynomial, R = max_degree in 1..d, d in 2..8.  The library evaluates k~ = k / S, S = sum_n sigma_n C(d, n) --
                       unit diagonal, values in [0, 1] like every other family --; the caller applies S as the `scale` of gpamd_kv_reduce_f32.  The
                       points are the ones gpamd_prep_points_f32 prepares for the BASE family (kind = base 0..3; stride round_up(d, 4), zero padding; d is an
                       explicit argument here, so no NaN padding).  The parameter block is rc device floats, rc = min(d, 3) when max_degree <= 3 and d
                       otherwise (the degree cap of the kernel that runs): block[n - 1] = sigma_n / S * 4096 (the 2^12 range shift of the split contraction
                       rides in the weights) for n <= max_degree, 0 above.  e_n is evaluated by the one-pass recursion with positive terms only, not by the
                       alternating Newton-Girard power sums.  float32 only.  Entry points: gpamd_kv_ng_partials_f32, gpamd_kv_ng_grad_f32 (+ its workspace query), which take
                       base, d and max_degree as arguments of their own, no `kind`.  Its product kernels ARE the additive kernels' body with the same tile,
                       launch bounds and waves per EU, so the launch is planned as the additive family's: gpamd_kv_plan(GPAMD_ADD, n, m, d, t,
                       GPAMD_KV_SPLIT, ...) gives S, jchunk and the workspace.  Every entry point that takes a `kind` refuses 9 as the unknown kind it was
                       before the family existed, gpamd_kv_plan included -- rows, dense blocks and diagonals of this family are the caller's
                       (backend.ng_cov).  Never culled.
                       Additive: the ABI version stays 5. */,
       GPAMD_GIBBS = 10 /* the Gibbs covariance with an input-dependent lengthscale l(x) > 0, the reference's GibbsKernel (gpytorch/kernels/gibbs_kernel.py:64-82,
                       which forms about six n x m tensors):  k(x, x') = sqrt(2 l(x) l(x') / (l(x)^2 + l(x')^2)) exp(-|x - x'|^2 / (l(x)^2 + l(x')^2)).
                       The exponent of the prefactor is 1/2 for EVERY d, as the reference executes it (Gibbs / Paciorek-Schervish have d/2): the matrix is
                       positive definite for d = 1 and in general NOT for d >= 2 with a varying l; one named constant per language holds it
                       (csrc/kv_directgibbs.hpp GIBBS_PREFACTOR_EXPONENT, families.GIBBS_PREFACTOR_EXPONENT).  No kparam, no block, no gpamd_prep_points_f32:
                       every parameter is PER POINT and sits in the rows, which the caller prepares (families.gibbs_prep), float32, 16-byte aligned,
                           row i = [ l_i^2 | 2^(1/4) sqrt(l_i) | x_i - shift (d columns) | zeros ],   width 4 (d <= 2) or 8 (d <= 6),
                       so a padding column adds nothing to the squared distance and the kernels exist in two widths only; the `d` of the entry points
                       is that WIDTH.  Unit diagonal, values in (0, 1].  A non-positive or non-finite l gives NaN, as in the reference: nothing is
                       checked.  Accepted by gpamd_kv_plan and gpamd_kv_partials_f32 (GPAMD_KV_SPLIT required; kparam ignored, X1c null, sq_cutoff 0: never
                       culled) and by gpamd_kv_gibbs_grad_f32 below, which has no `kind`; every other entry point refuses it -- rows, dense blocks and
                       diagonals are the caller's (families.gibbs_cov).  float32 only.  Additive: the ABI version stays 5. */,
       GPAMD_PS = 11 /* product structure over a parameter-free one-dimensional Matern base family -- the tensor-product (separable) Matern covariance, the
                       reference's ProductStructureKernel (gpytorch/kernels/product_structure_kernel.py:70-76, which forms a d x n x m tensor and multiplies it
                       down): k = prod_{q<d} k'(|x_q - x_q'|), k' in {Matern 1/2, 3/2, 5/2}, d in 2..8.  With r_q = |z_q - z_q'| in prepared units,
                       k = exp(-sum_q r_q) prod_q p_nu(r_q), p = 1, 1 + r, 1 + r + r^2 / 3: ONE exponential per pair whatever d, no square root.  Unit
                       diagonal (exact), values in (0, 1] like every other family; an outputscale is the caller's `scale` of gpamd_kv_reduce_f32.  The points
                       are the ones gpamd_prep_points_f32 prepares for the BASE family (kind = base 1..3; stride round_up(d, 4), zero padding; d is an explicit
                       argument here, so no NaN padding -- and a zero column would be neutral anyway: k'(0) = 1).  No kparam, no block.  base = 0 is refused: a
                       product of one-dimensional RBFs IS GPAMD_RBF with per-dimension lengthscales.  float32 only.  Entry points: gpamd_kv_ps_partials_f32,
                       gpamd_kv_ps_grad_f32 (+ its workspace query), which take base and d as arguments of their own, no `kind`.  Its product kernels ARE
                       the additive kernels' body with the same tile, launch bounds and waves per EU, so the launch is planned as the additive family's:
                       gpamd_kv_plan(GPAMD_ADD, n, m, d, t, GPAMD_KV_SPLIT, ...) gives S, jchunk and the workspace.  Every entry point that takes a `kind`
                       refuses 11 as the unknown kind it was before the family existed, gpamd_kv_plan included -- rows, dense blocks and diagonals of this
                       family are the caller's (families.ps_cov).  Never culled.  Additive: the ABI version stays 5. */,
       GPAMD_HAMMING = 12 /* the inverse-multiquadric Hamming covariance over fixed-length one-hot encoded sequences, the reference's HammingIMQKernel
                       (gpytorch/kernels/hamming_kernel.py:130-160, whose hamming_dist broadcasts an n x m x T x V tensor):
                       k = ((1 + alpha) / (alpha + c))^beta = k0 (1 + c / alpha)^(-beta) with c the Hamming distance in 0..T and k0 = ((1 + alpha) / alpha)^beta.
                       The kernels evaluate k~ = (1 + c / alpha)^(-beta) in (0, 1], exact unit diagonal; k0 is the caller's `scale` of gpamd_kv_reduce_f32.  No
                       gpamd_prep_points_f32: the caller prepares the rows (families.hamming_prep), float32-typed storage, 16-byte aligned,
                           row i = one BYTE per position, token + 1 in 1..127, four positions per dword, padded with the byte 1 to `width` dwords,
                       width 4, 8, 16 or 32 for T <= 16, 32, 64, 128 and a vocabulary of at most 126 letters.  Every dword is then a normal, finite float
                       bit pattern, and the count of differing positions of two dwords a, b is popcount(((a ^ b) + 0x7f7f7f7f) & 0x80808080).  alpha and
                       beta travel as the explicit arguments inv_alpha = 1 / alpha and beta.  float32 only.  Entry points: gpamd_kv_hamming_partials_f32,
                       gpamd_kv_hamming_grad_f32 (+ its workspace query), which take the width as an argument of their own, no `kind`.  Its product
                       kernels ARE the Gibbs kernels' body with the same tile, launch bounds, waves per EU and row-tile rule, so the launch is planned as
                       the Gibbs family's: gpamd_kv_plan(GPAMD_GIBBS, n, m, min(width, 8), t, GPAMD_KV_SPLIT, ...) gives S, jchunk and the workspace (none
                       of the three depends on the width).  Every entry point that takes a `kind` refuses 12 as the unknown kind it was before the family
                       existed, gpamd_kv_plan included -- rows, dense blocks and diagonals of this family are the caller's (families.hamming_cov).  Never
                       culled.  Additive: the ABI version stays 5. */ };
/* `kparam`: shape parameter of the parametrised covariance families (RQ: alpha > 0; PP: the code 4 j + q; ignored by the others), an EXPLICIT argument of
 * every entry point that evaluates the covariance or prepares points for it (ABI version 2: the library holds no per-thread kernel
 * state, so operators with different alpha may interleave freely on one thread -- AdditiveKernel(RQ, RQ)).  ABI version 3: the
 * float64 / generic entry points take it too (`double kparam`), so the family runs on every path.  ABI version 4 (additive): the block-Lanczos
 * vector entry points gpamd_block_{project,subtract,transform}_f32, and fused float32 kernels for input dimensions up to 32 (was 16).
 * ABI version 5 (additive): gpamd_kv_partials_far_f32 / gpamd_kv_far_workspace_ints -- the same product with far-pair tile culling --, its
 * derivative twins gpamd_kv_grad2_far_f32 / gpamd_kv_grad_far_f32, and the flag GPAMD_KV_SPLIT_FEW. */

enum { GPAMD_EINVAL = -1, GPAMD_EUNSUPPORTED = -2, GPAMD_EWORKSPACE = -3 };

/* kv flags.  GPAMD_KV_GRAM: the caller asserts max |z|^2 <= 32 over both prepared clouds (after centring) -- or passes block centres X1c, see gpamd_kv_partials_f32 --, so
 * the squared distances may be formed by the quadratic expansion on the matrix pipe (kv_gram.hpp; the expansion
 * the reference itself uses, gpytorch/kernels/kernel.py:26-49) with <= 2e-5 relative error in K (worst case at the limit; typically 5e-6).  Ignored for
 * Matern nu = 1/2. */
enum {
  GPAMD_KV_GRAM = 1,
  GPAMD_KV_WIDE = 2, /* tuning / A-B only: with GRAM, the pre-round-2 selection (no kv_gram4 / kv_gram16) */
  GPAMD_KV_G4 = 4,   /* tuning / A-B only: with GRAM, 9..12 columns on kv_gram4 instead of kv_gram16 */
  /* with GRAM, >= 5 columns: the contraction K * V runs on the f16 matrix pipe at f32 accuracy -- both operands split exactly
   * into f16 hi + lo parts (21-22 significant bits, power-of-two column scaling, f32 accumulation), three
   * v_mfma_f32_32x32x16_f16 in place of eight v_mfma_f32_32x32x2_f32 (kv_gramh.hpp).  The f16 planes of V live behind the
   * partial slabs of the workspace: size it with gpamd_kv_plan called with the same flags and pass the plan's jchunk (a multiple of
   * 128); the workspace must be 16-byte aligned and ldo a multiple of 4. */
  GPAMD_KV_SPLIT = 8,
  /* with GRAM and block centres X1c: the caller bounds the radius of 128-row aligned blocks only (not of the 256 / 512-row blocks the larger
   * row tilings centre): column groups of 5..65 columns with SPLIT run the split kernels at one row tile per wave (128 rows per workgroup),
   * every other column group takes the direct-difference kernels. */
  GPAMD_KV_BLOCK128 = 16,
  /* with SPLIT (ABI version 5): column groups of FEWER than five columns run on the split-operand kernels as well (one 32-column tile, mostly empty)
   * instead of the few-column kernels.  Slower when every tile is visited (the default selection stands for that reason); set by callers of
   * gpamd_kv_partials_far_f32, whose tile lists only the split-operand kernels walk: a one-column product of a numerically sparse K then skips the far
   * tiles too.  gpamd_kv_plan must be called with the same flags (the workspace holds the f16 planes of these groups). */
  GPAMD_KV_SPLIT_FEW = 32
};

int gpamd_abi_version(void);
const char* gpamd_last_error(void);

/* x / lengthscale (+ Matern mean-centring) -- gpytorch/kernels/rbf_kernel.py:78-79,
 * gpytorch/kernels/keops/rbf_kernel.py:45-46, keops/matern_kernel.py:69-71.
 * ls: nls = 1 (isotropic) or d (ARD) lengthscales; shift: d-vector or NULL. */
int gpamd_prep_points_f32(int kind, float kparam, const float* X, int n, int d, int64_t ldx, const float* ls, int nls,
                          const float* shift, float* Xp, int dp, void* stream);

/* Launch plan for one fused K*V: split count S and j-chunk so the grid is a whole number of chip fills of the
 * kernel variant that (kind, d, t, flags) selects.  Outputs on the host. workspace_floats = S * t * ldo (the partial slabs),
 * plus the split operand planes when flags carries GPAMD_KV_SPLIT. */
int gpamd_kv_plan(int kind, int n, int m, int d, int t, int flags, int64_t ldo, int* S_host, int* jchunk_host,
                  int64_t* workspace_floats_host);

/* P[s] = k(X1p, X2p[chunk s]) * Vt[:, chunk s]  for s < S -- the matrix-free K @ V of
 * KernelLinearOperator._matmul (gpytorch/kernels/keops/rbf_kernel.py:44-55) and
 * LazyEvaluatedKernelTensor._matmul (gpytorch/lazy/lazy_evaluated_kernel_tensor.py:245-275).
 * d: input dimension (1..32; the prepared clouds have stride dp = 4*ceil(d/4), 25..32 dimensions stride 32).
 * P: float[S][t][ldo].  done: optional device int; non-zero turns the launch into a no-op.
 * X1c (with GPAMD_KV_GRAM; NULL otherwise): float[ceil(n / 128)][dp], the centre of every 128-row chunk of X1p.  The Gram expansion is
 *   then taken relative to the centre of the workgroup's row block (squared distances are translation invariant), so its cancellation
 *   error scales with the BLOCK radius instead of the cloud radius -- the reference's Gram-trick distance has no scale limit
 *   (gpytorch/kernels/kernel.py:26-49).  The caller sorts the rows of X1p along a space-filling curve so that blocks are compact and
 *   asserts: max over 128 / 256 / 512-row aligned blocks (GPAMD_KV_BLOCK128: 128-row blocks) of |z - centre|^2 <= 32 and
 *   (max |z1| + max |z2|)^2 <= 2.5e7 (RQ: 60000 -- the split norm of a contracted point saturates at 60000, f16 range; every family but the
 *   heavy-tailed RQ is zero to f32 precision long before, gram_f16.hpp).  With X1c = NULL the GPAMD_KV_GRAM contract is the cloud-centred one (max |z|^2 <= 32).
 *   These are HARD preconditions of the flag, not hints: the kernels do not verify them (a check would cost a pass over both clouds per launch) and
 *   outside them entries of K lose accuracy silently.  A caller that cannot guarantee them passes flags without GPAMD_KV_GRAM (direct differences: no
 *   scale limit).  The Python host decides per product in backend.gram_mode / SortedView (tests/test_gpu_recenter.py: clouds at 0.8 of the extent limit). */
int gpamd_kv_partials_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt,
                          int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, int flags, const int* done,
                          void* stream);

/* The same product with FAR-PAIR TILE CULLING (opt-in; the reference evaluates every pair -- gpytorch/kernels/keops/rbf_kernel.py:44-55 leaves the
 * reduction over all j to KeOps -- and so does gpamd_kv_partials_f32).  For kernels whose mass sits within a few lengthscales (short lengthscales on
 * a wide cloud: the reference's 3droad workload starts at lengthscale 0.05 on z-scored inputs, examples/02_Scalable_Exact_GPs/KeOps_GP_Regression.ipynb)
 * most 128-point tiles of the contracted cloud hold no covariance above f32 resolution for a given block of output rows.  The caller orders BOTH
 * clouds along a space-filling curve (rows of X1p and of X2p, with Vt's columns in X2p's order) and passes bounding spheres:
 *   row_centres  float[ceil(n / 128)][dp], row_radii float[ceil(n / 128)]:  every 128-row aligned chunk of X1p lies within row_radii[q] of row_centres[q];
 *   tile_centres float[ceil(m / 128)][dp], tile_radii float[ceil(m / 128)]: the same for the 128-point aligned tiles of X2p;
 *   sq_cutoff: a squared distance in PREPARED coordinates (gpamd_prep_points_f32) beyond which the caller accepts k = 0.
 * A workgroup (128 .. 512 output rows: the union of its chunks' spheres) skips every tile of its j chunk whose sphere is farther than sqrt(sq_cutoff)
 * from its own; a skipped tile is neither loaded nor generated.  With sq_cutoff = s(eps), the squared distance at which the family's k falls to
 * eps, every dropped entry of K is <= eps, i.e. |(K V)_ic - culled| <= eps * sum_j |V_jc|.  sq_cutoff <= 0: exactly gpamd_kv_partials_f32 (the
 * other far arguments are ignored).  jchunk must be a multiple of 128 (gpamd_kv_plan's always is).  The spheres are taken on trust like the
 * GPAMD_KV_GRAM preconditions.  A small kernel builds, per column group, the list of surviving tiles of every (row block, j chunk) unit into
 * tile_workspace on the same stream; the product kernels walk the list.  Culled: the column groups that run on the split-operand kernels
 * (GPAMD_KV_SPLIT: kv_gramh.hpp, kv_directh.hpp -- the library's default contraction; groups of fewer than five columns only with
 * GPAMD_KV_SPLIT_FEW); every other group (fp32-MFMA contraction, the few-column kernels) evaluates every tile whatever is passed here -- exact,
 * only not faster.  All other arguments as gpamd_kv_partials_f32. */
int gpamd_kv_partials_far_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt,
                              int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, int flags, const int* done, void* stream,
                              const float* row_centres, const float* row_radii, const float* tile_centres, const float* tile_radii, float sq_cutoff,
                              int* tile_workspace, int64_t tile_workspace_ints);
/* ints of tile_workspace for a launch plan (S, jchunk) over n output rows: one list of (jchunk / 128 + 1) tile starts per (row block, j chunk). */
int64_t gpamd_kv_far_workspace_ints(int n, int S, int jchunk);

/* Out = scale * sum_s P[s] + (dscale + dvec) .* Vd  (scale/dscale device scalars, NULL = 1 / 0; dvec: optional
 * float[n] diagonal; Vd may be NULL): ScaleKernel.forward (gpytorch/kernels/scale_kernel.py:117-118) and the
 * + noise of _GaussianLikelihoodBase.marginal (gpytorch/likelihoods/gaussian_likelihood.py:117-121; dvec carries
 * FixedNoiseGaussianLikelihood's heteroskedastic diagonal, gaussian_likelihood.py:245-362). */
int gpamd_kv_reduce_f32(const float* P, int S, int64_t ldp, int t, int n, const float* scale, const float* dscale,
                        const float* dvec, const float* Vd, int64_t ldd, float* Out, int64_t ldo, const int* done,
                        void* stream);

/* One-call  Out = scale * K(X1p, X2p) Vt + dscale * Vd  using caller workspace (>= plan's workspace_floats). */
int gpamd_kv_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Vt, int64_t ldv,
                 int t, const float* scale, const float* dscale, const float* Vd, int64_t ldd, float* Out,
                 int64_t ldo, float* workspace, int64_t workspace_floats, int flags, void* stream);

/* Explicit entries (LinearOperator._getitem / _diagonal / to_dense on a kernel operator):
 * rows: out[r][j] = scale*k(X1p[rows[r]], X2p[j]);  dense: out[i][j] (row-major, ldo);  diag: out[i].
 * Before any launch: GPAMD_EINVAL for nrows / n / m / dp < 1 or ldo < m; GPAMD_EUNSUPPORTED for more than 65535 rows in one call (rows and dense:
 * the row is the grid's second extent -- callers go in blocks of 65535 rows, as the Python host does). */
int gpamd_kernel_rows_f32(int kind, float kparam, const float* X1p, const int64_t* rows, int nrows, const float* X2p, int m, int dp,
                          const float* scale, float* out, int64_t ldo, void* stream);
int gpamd_kernel_dense_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int dp, const float* scale,
                           float* out, int64_t ldo, void* stream);
int gpamd_kernel_diag_f32(int kind, float kparam, const float* X1p, const float* X2p, int n, int dp, const float* scale, float* out,
                          void* stream);

/* out[c] = sum_i A[c][i] * B[c][i]  (per-column inner products; scratch: float[t*256]) */
int gpamd_coldot_f32(const float* A, const float* B, int64_t ld, int n, int t, float* out, float* scratch,
                     void* stream);

/* ---- modified batched CG (linear_operator.utils.linear_cg; called from
 * gpytorch/distributions/multivariate_normal.py:249 and gpytorch/models/exact_prediction_strategies.py:286,444).
 * The handle only stores pointers into caller-owned device buffers. ---- */
typedef struct gpamd_cg gpamd_cg_t;

/* scratch sizes (in elements) for a t-column solve keeping hist_len iterations of (alpha, beta) */
int64_t gpamd_cg_fscratch_elems(int t, int hist_len);
int64_t gpamd_cg_iscratch_elems(int t);
/* offsets (in elements) of the host-visible pieces inside fscratch: bnorm, rnorm, alpha_hist, beta_hist, stats (each [t], the histories
 * [hist_len][t], stats [4]); the 2 t elements between rnorm and stats hold rho [2][t], the double-buffered r.z: iteration k reads half k & 1 and
 * writes the other */
int gpamd_cg_layout(int t, int hist_len, int64_t* offsets5_host);

/* X, R, D, Q: float[t][ld].  Z: float[t][ld] preconditioned residual, or == R without a preconditioner.
 * iscratch holds [zero_rhs(t) | converged(t) | done(2)]; done = {flag, iterations}. */
gpamd_cg_t* gpamd_cg_create_f32(int n, int t, int64_t ld, float* X, float* R, float* D, float* Q, float* Z,
                                float* fscratch, int* iscratch, int hist_len, float eps, float stop_updating_after);
void gpamd_cg_destroy(gpamd_cg_t* h);
const int* gpamd_cg_done_ptr(const gpamd_cg_t* h);

/* R = B/|B|, X = 0 (and D = R, rho = r.r when have_precond == 0) */
int gpamd_cg_init_f32(gpamd_cg_t* h, const float* B, int64_t ldb, int have_precond, void* stream);
/* with a preconditioner: after the caller wrote Z = P^-1 R and D = Z: rho = r.z */
int gpamd_cg_begin_f32(gpamd_cg_t* h, void* stream);
/* Row-sharded solves (each rank owns a contiguous block of rows of K_hat; used for the small-t solves
 * -- predictive-mean CG, Lanczos -- where probe-column sharding has nothing to split).  The solver's inner products
 * become sums over ranks: the three per-column partial arrays live in fscratch at offs[0..2] (d^T q, r^T z, r^T r), each
 * [t][stride] with nb used entries per column; between the producing and the consuming call the host sums a column's
 * partials, all-reduces the t sums (RCCL), writes them to entry 0 and zeroes the rest.  gpamd_cg_init_f32 is split at
 * those points: init_norms (-> offs[0]) | init_apply (-> offs[2], and offs[1] when copy_d) | begin_apply. */
int gpamd_cg_partials_layout(int n, int t, int hist_len, int64_t* offs, int* stride, int* nb);
int gpamd_cg_init_norms_f32(gpamd_cg_t* h, const float* B, int64_t ldb, void* stream);
int gpamd_cg_init_apply_f32(gpamd_cg_t* h, const float* B, int64_t ldb, int copy_d, void* stream);
int gpamd_cg_begin_apply_f32(gpamd_cg_t* h, void* stream);
/* preconditioned row-sharded solves: gpamd_cg_begin_f32 / gpamd_cg_update_d_f32 split at the r^T z partial sums --
 * dot_rz writes the per-workgroup partials of r^T z (layout: gpamd_cg_partials_layout, offs[1]); the host all-reduces them;
 * begin_apply / update_d_apply consume them. */
int gpamd_cg_dot_rz_f32(gpamd_cg_t* h, void* stream);
int gpamd_cg_update_d_apply_f32(gpamd_cg_t* h, int k, void* stream);
/* Q = scale * sum_s P[s] + (dscale + dvec) .* D, and d.q partials */
int gpamd_cg_reduce_q_f32(gpamd_cg_t* h, const float* P, int S, int64_t ldp, const float* scale, const float* dscale,
                          const float* dvec, void* stream);
/* alpha; X += alpha D; R -= alpha Q.   k (here, in update_d and in stop): the iteration index, or -1 = take it from the device
 * (the count cg_stop maintains) -- the form to record into a hipGraph that is then replayed once per iteration. */
int gpamd_cg_update_xr_f32(gpamd_cg_t* h, int k, void* stream);
/* (caller applies Z = P^-1 R here when preconditioned)  beta; D = Z + beta D; residual statistics -> stats */
int gpamd_cg_update_d_f32(gpamd_cg_t* h, int k, void* stream);
/* stopping rule on stats (all-reduce stats[0:2] across ranks first when probe columns are sharded) */
int gpamd_cg_stop_f32(gpamd_cg_t* h, int k, int min_iter, int tridiag_floor, float tol, void* stream);
/* ---- RCCL-communicator variants ("RCCL communicator handle passed in for the multi-GPU variants"; they replace the peer
 * copies of gpytorch/kernels/multi_device_kernel.py:49-92).  rccl_comm: an ncclComm_t of the caller (one rank per GPU); stream-ordered on
 * `stream`, no host round trip.  librccl.so is resolved on first use (dlopen), so single-GPU hosts need not have it.
 *   gpamd_cg_stop_comm_f32: the stopping rule of a PROBE-SHARDED solve -- all-reduces the solver's two residual statistics (sum of column
 *     residual norms, column count) over the communicator, then applies the rule: the ONLY per-iteration collective of the design.
 *   gpamd_allreduce_sum_f32: in-place sum of `count` device floats (SLQ partial sums, packed hyper-parameter gradients, the k x t
 *     preconditioner coefficients of a row-sharded apply).
 * The Python host of this repository drives the same collectives through torch.distributed (backend "nccl" = RCCL), which owns its
 * communicators; these entry points serve hosts that hold an ncclComm_t themselves. ---- */
int gpamd_cg_stop_comm_f32(gpamd_cg_t* h, int k, int min_iter, int tridiag_floor, float tol, void* rccl_comm, void* stream);
int gpamd_allreduce_sum_f32(float* buf, int64_t count, void* rccl_comm, void* stream);
/* X *= |B| */
int gpamd_cg_finish_f32(gpamd_cg_t* h, void* stream);

/* ---- pivoted Cholesky of the NOISE-FREE kernel matrix (LinearOperator.pivoted_cholesky; wrapper
 * gpytorch/__init__.py:146-173; consumer AddedDiagLinearOperator._preconditioner). L: float[rank][ldl]
 * (zero-filled by the caller), rank <= 512; fwork: float[n + 4]; iwork: int[2 + 2n]; pivots: int64[rank].
 * Runs `rank` (pivot, update) steps without host synchronisation; steps after the error tolerance is
 * met are no-ops.  On completion iwork[0] = number of columns produced. ---- */
int gpamd_pivoted_cholesky_f32(int kind, float kparam, const float* Xp, int n, int dp, const float* scale, int rank, float tol,
                               float* L, int64_t ldl, int64_t* pivots, float* fwork, int* iwork, void* stream);

/* ---- Lanczos tridiagonalisation with full re-orthogonalisation: the vector work of one step (float32 vectors of length n,
 * basis Q [k][ldq] probe-major).  Replaces the torch GEMV / norm chain of linear_operator.utils.lanczos.lanczos_tridiag
 * (reached from gpytorch/models/exact_prediction_strategies.py:202,234-238,271); the operator product w = K_hat q is
 * gpamd_kv_partials_f32 + gpamd_kv_reduce_f32 with t = 1.  All scalars stay on the device; partial sums are
 * [k][gpamd_lanczos_partial_stride()] floats with gpamd_lanczos_num_partials(n) valid entries per row, finished in a fixed order
 * by gpamd_lanczos_coef_f32 (row-sharded callers all-reduce `coef` between coef and subtract / normalize).
 *   residual : r = w - beta_prev[0] * q_prev            (q_prev == NULL: r = w)
 *   project  : part[m][b] = partial <Q[m], r>, m < k <= 512
 *   coef     : coef[m] = sum_b part[m][b]; tol >= 0: flag[0] |= (|coef[m]| > tol)
 *   subtract : r -= sum_m coef[m] Q[m]; part_rr[b] = partial |r|^2       (finish with gpamd_lanczos_coef_f32(part_rr, 1, ...))
 *   normalize: out = r / sqrt(max(rr[0], 0)) (exact zeros when that is 0); norm_out[0] = the norm; stop[0] |= (norm < tiny); norm_out, stop: may be NULL
 * Limits, GPAMD_EINVAL before any launch: project / subtract take k <= 512 basis rows, ldq >= n and ldq % 4 == 0 (every row 16-byte aligned, as w, r, out
 * must be); coef takes nb <= gpamd_lanczos_partial_stride() and, for tol >= 0, a non-NULL flag. ---- */
int gpamd_lanczos_num_partials(int n);
int gpamd_lanczos_partial_stride(void);
int gpamd_lanczos_residual_f32(const float* w, const float* q_prev, const float* beta_prev, float* r, int n, void* stream);
int gpamd_lanczos_project_f32(const float* Q, int64_t ldq, int k, const float* r, int n, float* part, void* stream);
int gpamd_lanczos_coef_f32(const float* part, int k, int nb, float tol, float* coef, int* flag, void* stream);
int gpamd_lanczos_subtract_f32(const float* Q, int64_t ldq, int k, const float* coef, float* r, int n, float* part_rr, void* stream);
int gpamd_lanczos_normalize_f32(const float* r, int n, const float* rr, float* out, float* norm_out, float tiny, int* stop, void* stream);

/* ---- BLOCK Lanczos with full re-orthogonalisation: the vector work of one step for a block of b probe-major rows R [b][ldr] against a basis
 * Q [k][ldq] of ANY length k (float32 vectors, float64 accumulation).  Limits, GPAMD_EINVAL before any launch: subtract and transform take b <= 32
 * (project takes any b); ldq >= n and ldr >= n, no alignment asked of either (scalar loads).  Behind LinearOperator.root_inv_decomposition (the LOVE covar_cache,
 * gpytorch/models/exact_prediction_strategies.py:267-272) and the multi-vector form of gpytorch.root_inv_decomposition (gpytorch/__init__.py:190-216): the b
 * vectors ride through ONE b-column gpamd_kv_partials_f32 per step instead of b single-column products.
 *   project  : W[c][m] = <R[c], Q[m]>                  W: double [b][k]; ANY b (column groups of 16); workspace: double[gpamd_precond_coef_workspace_doubles(n, min(b, 16), k)].
 *              With R = Q it is the Gram matrix of tall-skinny rows -- the two Gram products of the preconditioner's Cholesky-QR
 *              (AddedDiagLinearOperator._preconditioner's QR of [L; sigma I]; rocBLAS' float64 GEMM takes 35 ms for the 15 x 217 437 x 15 shape); _f64: both
 *              operands double (the second Cholesky-QR pass)
 *   subtract : R[c] -= sum_m W[c][m] Q[m]              (in place)
 *   transform: R[r] = sum_c M[r][c] R[c]               (in place; M: double [b][b], e.g. the inverse Cholesky factor of R R^T: Cholesky-QR) ---- */
int gpamd_block_project_f32(const float* Q, int64_t ldq, int k, const float* R, int64_t ldr, int b, int n, double* W, double* workspace,
                            int64_t workspace_doubles, void* stream);
int gpamd_block_project_f64(const double* Q, int64_t ldq, int k, const double* R, int64_t ldr, int b, int n, double* W, double* workspace,
                            int64_t workspace_doubles, void* stream);
int gpamd_block_subtract_f32(const float* Q, int64_t ldq, int k, const double* W, float* R, int64_t ldr, int b, int n, void* stream);
int gpamd_block_transform_f32(const double* M, float* R, int64_t ldr, int b, int n, void* stream);

/* ---- multi-shift MINRES (contour-integral quadrature: gpytorch.sqrt_inv_matmul, gpytorch/__init__.py:252-278 ->
 * linear_operator.utils.minres; consumer variational/ciq_variational_strategy.py:217): the vector part of ONE iteration for all Q shifts:
 * d = (v_c - delta d1 - eps d2) / gamma written over d2 (the caller swaps the two direction buffers), x += tau d.
 * v: [t][ld]; d1, d2, x: [Q][t][ld]; coef: float[4][Q][t] = delta | eps | 1 / gamma | tau (device). ---- */
int gpamd_msminres_update_f32(const float* v, const float* d1, float* d2, float* x, const float* coef, int Q, int t, int n, int64_t ld,
                              void* stream);

/* ---- pivoted-Cholesky preconditioner apply, first half:  W[c][m] = sum_i R[c][i] * Q1[m][i]  with R float32 [t][ldr] (the CG
 * residuals), Q1 float64 [k][ldq] (k <= 512: GPAMD_EINVAL beyond, in both halves), W float64 [t][k], float64 accumulation -- the k x t coefficients of
 * AddedDiagLinearOperator._preconditioner's closure  P^-1 R = (R - Q1 Q1^T R) / sigma^2, whose cancellation float32 cannot carry
 * (gpytorch_amd/linear_cg.py).  workspace: double[gpamd_precond_coef_workspace_doubles(n, t, k)]; fewer: GPAMD_EWORKSPACE. ---- */
int64_t gpamd_precond_coef_workspace_doubles(int n, int t, int k);
int gpamd_precond_coef_f32f64(const float* R, int64_t ldr, int t, const double* Q, int64_t ldq, int k, int n, double* W,
                              double* workspace, int64_t workspace_doubles, void* stream);
/* second half, fused:  Out[c][i] = (R[c][i] - sum_m W[c][m] Q1[m][i]) / sigma2[0]  (float64 arithmetic, float32 in / out; Out may
 * alias nothing but itself -- R and Out are different buffers in the mBCG state).  sigma2: one float on the device. */
int gpamd_precond_apply_f32f64(const float* R, int64_t ldr, int t, const double* Q, int64_t ldq, int k, int n, const double* W,
                               const float* sigma2, float* Out, int64_t ldo, void* stream);

/* ---- fused bilinear derivative: out[0] = sum_ij W_ij k_ij, out[1+q] = sum_ij W_ij dk/ds_ij (z_iq - z_jq)^2,
 * W = Lt^T Rt (never formed).  Replaces LinearOperator._bilinear_derivative on the kernel operator and the
 * dense backward of gpytorch/functions/rbf_covariance.py:26-29 / matern_covariance.py:53-56 (chunked variant:
 * gpytorch/lazy/lazy_evaluated_kernel_tensor.py:69-104).  out: float[1 + dp]; workspace: double[>= the query].
 * iso != 0 (single lengthscale): out[1] = sum_ij W_ij dk/ds_ij s_ij and out[2..] = 0 (cheaper epilogue). ---- */
int64_t gpamd_kv_grad_workspace_doubles(int n, int m, int t, int dp);
int gpamd_kv_grad_f32(int kind, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                      const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                      int64_t workspace_doubles, void* stream);

/* ---- the same derivative with Gram-form generation (squared distances on the matrix pipe, kv_grad2.hpp) and, optionally,
 * the gradient with respect to the PREPARED left points:  Gz1t[q][i] = sum_j W_ij dk/ds_ij * 2 (z_iq - z_jq)  (probe-major
 * [d][ldg]; the caller applies dz/dx = coef / lengthscale_q and theta -- the input gradients the KeOps precedent provides,
 * gpytorch/test/base_keops_test_case.py:105-132; the reference's dense Functions refuse them, rbf_covariance.py:9-10).
 * RBF / Matern 3/2 / Matern 5/2 / RQ only, accurate while max |z|^2 <= 32 or, with block centres X1c (as for gpamd_kv_partials_f32), while the
 * block radius^2 <= 8 (the host's policy for every Gram-form kernel); d = valid
 * dimensions (points are [n][round_up(d,4)]).  out: float[2 + round_up(d,4)]: [0 .. dp] as gpamd_kv_grad_f32, [1 + dp] = sum_ij W_ij dk/dp_ij at
 * fixed s for the family's shape parameter (RQ alpha; 0 otherwise).  Gz1t == NULL: hyper-parameters only (xworkspace unused). ---- */
int64_t gpamd_kv_grad2_workspace_doubles(int n, int m, int t, int d);
int64_t gpamd_kv_grad2_xworkspace_floats(int n, int m, int t, int d);
/* flags & GPAMD_KV_SPLIT: the W = L^T R contraction runs on the f16 matrix pipe at f32 accuracy (hi/lo-split planes of both vector blocks,
 * per-column power-of-two scales with a constant product; kv_wsplit.hpp) -- 15 v_mfma_f32_32x32x16_f16 per 32 x 32 tile instead of 33
 * v_mfma_f32_32x32x2_f32 at 65 columns.  Needs sworkspace (16-byte aligned, gpamd_kv_grad2_split_workspace_floats floats); the plain
 * workspaces sized for the same t cover either path. */
int64_t gpamd_kv_grad2_split_workspace_floats(int n, int m);
int gpamd_kv_grad2_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Lt, int64_t ldl,
                       const float* Rt, int64_t ldr, int t, int iso, float* out, float* Gz1t, int64_t ldg, double* workspace,
                       int64_t workspace_doubles, float* xworkspace, int64_t xworkspace_floats, int flags, float* sworkspace,
                       int64_t sworkspace_floats, void* stream);

/* The two derivative kernels with FAR-PAIR TILE CULLING (ABI version 5; contract, spheres and bound as gpamd_kv_partials_far_f32: both clouds and their
 * vector blocks in curve order, bounding spheres of the 128-point chunks, sq_cutoff the squared prepared distance beyond which k -- and with it dk/ds --
 * is accepted as zero; sq_cutoff <= 0: exactly the un-culled entry points).  A (128-row block, j chunk) unit skips the 64-row j steps whose 128-point
 * tile lies farther than sqrt(sq_cutoff) from its rows: neither the W tile nor the covariance derivative of a skipped step is formed.  The sums are
 * order-free, so the caller need not take anything back to the original order (Gz1t comes out in X1p's order, as always).
 * tile_workspace: gpamd_kv_grad2_far_workspace_ints(n, m) / gpamd_kv_grad_far_workspace_ints(n, m) ints. */
int64_t gpamd_kv_grad2_far_workspace_ints(int n, int m);
int gpamd_kv_grad2_far_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int d, const float* X1c, const float* Lt, int64_t ldl,
                           const float* Rt, int64_t ldr, int t, int iso, float* out, float* Gz1t, int64_t ldg, double* workspace,
                           int64_t workspace_doubles, float* xworkspace, int64_t xworkspace_floats, int flags, float* sworkspace,
                           int64_t sworkspace_floats, void* stream, const float* row_centres, const float* row_radii, const float* tile_centres,
                           const float* tile_radii, float sq_cutoff, int* tile_workspace, int64_t tile_workspace_ints);
int64_t gpamd_kv_grad_far_workspace_ints(int n, int m);
int gpamd_kv_grad_far_f32(int kind, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                          const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                          int64_t workspace_doubles, void* stream, const float* row_centres, const float* row_radii, const float* tile_centres,
                          const float* tile_radii, float sq_cutoff, int* tile_workspace, int64_t tile_workspace_ints);
/* gpamd_kv_grad_far_f32 for the families whose covariance needs `kparam` and has no learnable shape parameter -- the piecewise polynomial, every q:
 * the direct-difference derivative is what serves its q = 0 (a cusp at r = 0, as Matern nu = 1/2) and the rows outside the Gram policy.  Additive:
 * ABI version 5 stands; GPAMD_RBF .. GPAMD_MATERN52 are accepted too (kparam ignored); GPAMD_RQ is not (no shape-parameter sum comes out). */
int gpamd_kv_grad_param_far_f32(int kind, float kparam, const float* X1p, int n, const float* X2p, int m, int dp, const float* Lt, int64_t ldl,
                                const float* Rt, int64_t ldr, int t, int iso, float* out, double* workspace,
                                int64_t workspace_doubles, void* stream, const float* row_centres, const float* row_radii,
                                const float* tile_centres, const float* tile_radii, float sq_cutoff, int* tile_workspace,
                                int64_t tile_workspace_ints);

/* ---- spectral-mixture family (GPAMD_SM above has the formula, the prepared row and the parameter block).
 * gpamd_kv_sm_partials_f32: gpamd_kv_partials_f32 for this family (same slabs, same plan -- gpamd_kv_plan with kind = GPAMD_SM, d = width, GPAMD_KV_SPLIT --
 * same done flag; the slabs hold k~ V, reduce them with scale = Wsum^d).  GPAMD_EUNSUPPORTED: (q, d) outside the envelope; GPAMD_EINVAL: null block,
 * width != d + 2 q d, and what gpamd_kv_partials_f32 refuses -- all before any launch.
 * gpamd_kv_sm_grad_f32: out[1 + 3 q d] = the bilinear-derivative sums with W = Lt^T Rt (as gpamd_kv_grad_f32), tau_j = x_ij - x_jj, e = exp(-2 pi^2
 * sigma_qj^2 tau_j^2), rest~_j = prod_{j' != j} f~_j', u = q d + j:
 *   out[0] = sum W k~;   out[1 + u] = sum W rest~_j w^_q e cos;   out[1 + q d + u] = sum W rest~_j w^_q e cos tau_j^2;   out[1 + 2 q d + u] = sum W rest~_j w^_q e sin tau_j
 * (float64 accumulation in `workspace`, gpamd_kv_sm_grad_workspace_doubles doubles).  With k = s k~, s = Wsum^d held fixed:
 *   dk/dsigma_qj = -4 pi^2 sigma_qj s out[1 + q d + u],  dk/dmu_qj = -2 pi s out[1 + 2 q d + u],  dk/dw_q = s / Wsum (sum_j out[1 + u] / w^_q - d out[0]). */
int gpamd_kv_sm_partials_f32(const float* block, int q, int d, const float* X1p, int n, const float* X2p, int m, int width, const float* Vt, int64_t ldv,
                             int t, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_sm_grad_workspace_doubles(int n, int m, int t, int q, int d);
int gpamd_kv_sm_grad_f32(const float* block, int q, int d, const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- Newton-Girard additive family (GPAMD_NG above has the formula, the normalisation and the weight block; rc = min(d, 3) if max_degree <= 3, else d).
 * gpamd_kv_ng_partials_f32: gpamd_kv_partials_f32 for this family (same slabs, same done flag; the plan is gpamd_kv_plan's for kind = GPAMD_ADD at the same
 * d with GPAMD_KV_SPLIT: the two families share kernel body, tile geometry and launch bounds; the slabs hold k~ V, reduce them with scale = S).  GPAMD_EUNSUPPORTED: d outside 2..8; GPAMD_EINVAL: null block, base outside 0..3, max_degree
 * outside 1..d, and what gpamd_kv_partials_f32 refuses -- all before any launch.
 * gpamd_kv_ng_grad_f32: out[1 + d + rc] = the bilinear-derivative sums with W = Lt^T Rt (as gpamd_kv_grad_f32), s_q = (z_iq - z_jq)^2 in prepared units,
 * w_n = sigma_n / S:
 *   out[0] = sum W k~;   out[1 + q] = sum W (sum_n w_n e_{n-1}(z without z_q)) (dk'/ds)(s_q) s_q;   out[1 + d + n - 1] = sum W e_n(z),  n = 1..rc
 * (float64 accumulation in `workspace`, gpamd_kv_ng_grad_workspace_doubles doubles; the leave-one-out polynomials by the adjoint of the recursion, no
 * quotient by z_q).  With k = sum_n sigma_n e_n:   dk/dsigma_n = out[1 + d + n - 1],   dk/dl_q = S out[1 + q] (-2 / l_q). */
int gpamd_kv_ng_partials_f32(const float* block, int base, int d, int max_degree, const float* X1p, int n, const float* X2p, int m, const float* Vt,
                             int64_t ldv, int t, float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_ng_grad_workspace_doubles(int n, int m, int t, int d, int max_degree);
int gpamd_kv_ng_grad_f32(const float* block, int base, int d, int max_degree, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                         const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- Gibbs family (GPAMD_GIBBS above has the formula and the row layout; `width` = the prepared width, 4 or 8).  The product is gpamd_kv_partials_f32 with
 * kind = GPAMD_GIBBS and d = width, planned by gpamd_kv_plan with the same arguments.
 * gpamd_kv_gibbs_grad_f32: with W = Lt^T Rt (as gpamd_kv_grad_f32) and, per pair, u^2 = 1 / (l_i^2 + l_j^2), s = |x_i - x_j|^2,
 *   out[0]     = sum_ij W_ij k_ij
 *   out[1 + i] = sum_j  W_ij dk_ij/dl_i,   dk/dl_i = k (1 / (2 l_i) - l_i u^2 + 2 s l_i u^4),     i = 0 .. n - 1          (out: 1 + n floats)
 * -- the gradient with respect to the lengthscale of EVERY point of the first cloud; for the second cloud's, call it with the clouds and Lt, Rt
 * exchanged (dk/dl_j is the same expression with i and j exchanged); for one cloud against itself the total derivative is the sum of the two calls.
 * Per-row sums are accumulated per lane and stored once per row and chunk of the contracted index, then summed in float64 in a fixed order: no
 * atomics, two calls give the same bits.  `workspace`: gpamd_kv_gibbs_grad_workspace_doubles doubles (0: arguments it refuses).  GPAMD_EUNSUPPORTED: width
 * not 4 or 8; GPAMD_EINVAL: a null pointer, n, m or t < 1, ldl < n, ldr < m; GPAMD_EWORKSPACE: workspace too small -- all before any launch. */
int64_t gpamd_kv_gibbs_grad_workspace_doubles(int n, int m, int t, int width);
int gpamd_kv_gibbs_grad_f32(const float* X1p, int n, const float* X2p, int m, int width, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t,
                            float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- Product-structure family = tensor-product Matern (GPAMD_PS above has the formula and the prepared rows).
 * gpamd_kv_ps_partials_f32: gpamd_kv_partials_f32 for this family (same slabs, same done flag; the plan is gpamd_kv_plan's for kind = GPAMD_ADD at the same
 * d with GPAMD_KV_SPLIT: the two families share kernel body, tile geometry and launch bounds).  GPAMD_EUNSUPPORTED: d outside 2..8; GPAMD_EINVAL: base
 * outside 1..3 (base = 0 with a text that names the RBF family with per-dimension lengthscales), and what gpamd_kv_partials_f32 refuses -- all before
 * any launch.
 * gpamd_kv_ps_grad_f32: out[1 + d] = the bilinear-derivative sums with W = Lt^T Rt (as gpamd_kv_grad_f32), r_q = |z_iq - z_jq| in prepared units:
 *   out[0] = sum W k;   out[1 + q] = sum W k rho_q,   rho_q = (dk'/ds)(s_q) s_q / k'(s_q) at s_q = r_q^2
 *          = -r/2 (nu = 1/2),  -r^2 / (2 (1 + r)) (nu = 3/2),  -r^2 (1 + r) / (6 (1 + r + r^2 / 3)) (nu = 5/2)
 * (float64 accumulation in `workspace`, gpamd_kv_ps_grad_workspace_doubles doubles, fixed order, no atomics: two calls give the same bits; an exact zero
 * at r_q = 0).  dk/dl_q = scale out[1 + q] (-2 / l_q).  GPAMD_EUNSUPPORTED: d outside 2..8; GPAMD_EINVAL: a bad base, null pointers, bad extents;
 * GPAMD_EWORKSPACE: a workspace smaller than the query's. */
int gpamd_kv_ps_partials_f32(int base, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t, float* P, int64_t ldo,
                             int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_ps_grad_workspace_doubles(int n, int m, int t, int d);
int gpamd_kv_ps_grad_f32(int base, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl, const float* Rt, int64_t ldr, int t,
                         float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- Hamming family over packed tokens (GPAMD_HAMMING above has the formula and the prepared rows; `width` = the prepared width in dwords: 4, 8, 16, 32).
 * Replaces gpytorch/kernels/hamming_kernel.py:146-160 (hamming_dist: x1.unsqueeze(-3) * x2.unsqueeze(-4), an n x m x T x V tensor, and _imq on the n x m
 * distances) and, for the derivative, the autograd graph through both.
 * gpamd_kv_hamming_partials_f32: gpamd_kv_partials_f32 for this family (same slabs, same done flag; the plan is gpamd_kv_plan's for kind = GPAMD_GIBBS at
 * d = min(width, 8) with GPAMD_KV_SPLIT: the two families share kernel body, tile geometry, launch bounds and row-tile rule).  GPAMD_EUNSUPPORTED: a width
 * other than 4, 8, 16, 32; GPAMD_EINVAL: inv_alpha or beta not positive and finite, and what gpamd_kv_partials_f32 refuses -- all before any launch.
 * gpamd_kv_hamming_grad_f32: out[3] = the bilinear-derivative sums with W = Lt^T Rt (as gpamd_kv_grad_f32), s = c / alpha, k~ = (1 + s)^(-beta):
 *   out[0] = sum W k~;   out[1] = sum W s dk~/ds = sum W k~ (-beta s / (1 + s));   out[2] = sum W dk~/dbeta at fixed s = sum W k~ (-ln(1 + s))
 * (float64 accumulation in `workspace`, gpamd_kv_hamming_grad_workspace_doubles doubles, fixed order, no atomics: two calls give the same bits; exact
 * zeros in out[1], out[2] from pairs with c = 0).  d k~/d alpha = -out[1] / alpha.  GPAMD_EUNSUPPORTED: a bad width; GPAMD_EINVAL: bad parameters, null
 * pointers, bad extents; GPAMD_EWORKSPACE: a workspace smaller than the query's. */
int gpamd_kv_hamming_partials_f32(int width, float inv_alpha, float beta, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                  float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_hamming_grad_workspace_doubles(int n, int m, int t, int width);
int gpamd_kv_hamming_grad_f32(int width, float inv_alpha, float beta, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                              const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- RBF kernel with derivative observations (the reference's RBFKernelGrad, gpytorch/kernels/rbf_kernel_grad.py:60-104): the n (d + 1) x m (d + 1)
 * operator over values and gradients, never formed.  Interleaved layout: entry i (d + 1) + a of a vector is component a of point i, a = 0 the value,
 * a = 1..d the partial derivatives, so a column of Vt / P / Lt / Rt is [points][d + 1] floats and its leading dimension is >= points (d + 1).
 * X1p / X2p are the points gpamd_prep_points_f32 prepares for GPAMD_RBF (stride 4: d <= 4; its shift included); inv_ls: d device floats 1 / l_a (one
 * lengthscale: d equal entries).  With delta = (x_i - x_j) / l, k = exp(-|delta|^2 / 2), r~_b = r_b / l_b:
 *   q_ij = r_j0 + delta . r~_j;   out_i0 = sum_j k q_ij;   out_ia = (1 / l_a) sum_j k (r~_ja - delta_a q_ij)
 * gpamd_kv_rbfgrad_plan: S, jchunk and the S t ldo floats of the slabs.  gpamd_kv_rbfgrad_partials_f32: P [S][t][ldo], the slabs of
 * gpamd_kv_partials_f32 (same done flag; sum them with gpamd_kv_reduce_f32 / gpamd_cg_reduce_q over n (d + 1) entries -- the outputscale and the
 * diagonal ride there); more than four columns run as groups of four.  gpamd_kv_rbfgrad_grad_f32: with p_ij = l_i0 - delta . l~_i and
 * f_ij = p q + l~_i . r~_j, summed over all pairs and the t column pairs (Lt [t][ldl] over X1p, Rt [t][ldr] over X2p; float64 accumulation in
 * `workspace`, gpamd_kv_rbfgrad_grad_workspace_doubles doubles):
 *   out[0] = sum k f  (= sum_c l_c^T K r_c: the outputscale gradient);
 *   out[1 + a] = sum k [ -delta_a^2 f + 2 delta_a (p r~_ja - l~_ia q) + 2 l~_ia r~_ja ],   d(sum_c l_c^T K r_c) / d l_a = -out[1 + a] / l_a.
 * GPAMD_EUNSUPPORTED: d outside 1..4; GPAMD_EINVAL: a null pointer, a leading dimension below points (d + 1), a jchunk that is not the plan's;
 * GPAMD_EWORKSPACE: too few doubles -- all before any launch. */
int gpamd_kv_rbfgrad_plan(int n, int m, int d, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_floats);
int gpamd_kv_rbfgrad_partials_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                  float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_rbfgrad_grad_workspace_doubles(int n, int m, int d);
int gpamd_kv_rbfgrad_grad_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                              const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- Matern-5/2 kernel with derivative observations (the reference's Matern52KernelGrad, gpytorch/kernels/matern52_kernel_grad.py:102-196): the
 * twin of the RBF entry points above -- same layout, same arguments, same plan, slabs, reduce and error codes -- on the points gpamd_prep_points_f32
 * prepares for GPAMD_MATERN52 (stride 4: d <= 4).  With delta = (x_i - x_j) / l, rho = |delta|^2, s = sqrt(5 rho), e = exp(-s) the radial factors are
 *   k = (1 + s + s^2 / 3) e,   g = (5/3) (1 + s) e = -2 dk/drho,   w = (25/3) e = -2 dg/drho,   u = (125/3) e / s = -2 dw/drho  (0 for s < 1e-6)
 * (RBF is k = g = w = u = exp(-rho / 2)) and the block of a pair is
 *   K[i0, j0] = k;  K[i0, jb] = g delta_b / l_b;  K[ia, j0] = -g delta_a / l_a;  K[ia, jb] = (g [a = b] - w delta_a delta_b) / (l_a l_b).
 * Product, with r~_b = r_b / l_b and B = delta . r~_j:
 *   out_i0 = sum_j [ k r_j0 + g B ];   out_ia = (1 / l_a) sum_j [ g r~_ja - delta_a (g r_j0 + w B) ]
 * Bilinear derivative, with l~_a = l_a / l_a-th lengthscale, A = delta . l~_i, C = l~_i . r~_j, M = l_i0 B - r_j0 A + C:
 *   out[0] = sum [ k l0 r0 + g M - w A B ]  (= sum_c l_c^T K r_c: the outputscale gradient);
 *   out[1 + a] = -sum [ delta_a^2 (g l0 r0 + w M - u A B) - 2 g (delta_a (l0 r~_a - r0 l~_a) + l~_a r~_a) + 2 w delta_a (l~_a B + r~_a A) ],
 *   d(sum_c l_c^T K r_c) / d l_a = -out[1 + a] / l_a   (the sign of the RBF entry point: one host assembly serves both). */
int gpamd_kv_m52grad_plan(int n, int m, int d, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_floats);
int gpamd_kv_m52grad_partials_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                  float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_m52grad_grad_workspace_doubles(int n, int m, int d);
int gpamd_kv_m52grad_grad_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                              const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- RBF kernel with first- and second-derivative observations (the reference's RBFKernelGradGrad, gpytorch/kernels/rbf_kernel_gradgrad.py:60-151):
 * the n (2 d + 1) x m (2 d + 1) operator over values, gradients and the d non-mixed second partial derivatives, never formed.  The twin of the
 * gpamd_kv_rbfgrad_* entry points -- same prepared points (GPAMD_RBF, stride 4: d <= 4), inv_ls, plan, slabs, done flag, reduce and error codes -- with
 * C = 2 d + 1 floats per point in every column: entry i C + c is the value (c = 0), d/dx_a (c = a, 1 <= a <= d) or d2/dx_a^2 (c = d + a) of point i,
 * and leading dimensions are >= points (2 d + 1).  With u_q = (x_iq - x_jq) / l_q, k = exp(-|u|^2 / 2), derivative orders alpha, beta in
 * {0, e_a, 2 e_a} of the row and the column component and the probabilists' Hermite polynomials He_n (He_1 = u, He_2 = u^2 - 1, He_3 = u^3 - 3u,
 * He_4 = u^4 - 6u^2 + 3, ...):
 *   K[(i, alpha), (j, beta)] = k prod_q (-1)^{alpha_q} He_{alpha_q + beta_q}(u_q) / l_q^{alpha_q + beta_q}
 * Product, with r~1_a = r_ja / l_a, r~2_a = r_j,d+a / l_a^2 and S0 = r_j0 + sum_q [ u_q r~1_q + He_2(u_q) r~2_q ]:
 *   out_i0 = sum_j k S0;   out_ia = (1 / l_a) sum_j k [ -u_a S0 + r~1_a + 2 u_a r~2_a ];
 *   out_i,d+a = (1 / l_a^2) sum_j k [ He_2(u_a) S0 - 2 u_a r~1_a + (2 - 4 u_a^2) r~2_a ]
 * More columns than the widest instantiation (four for d <= 3, two for d = 4) run as groups.  gpamd_kv_rbfgradgrad_grad_f32, summed over all pairs
 * and the t column pairs, with K^(a) the block in which He_s(u_a), s = alpha_a + beta_a, is replaced by He_{s+2}(u_a) + He_s(u_a):
 *   out[0] = sum l^T K r  (the outputscale gradient);   out[1 + a] = -sum l^T K^(a) r,   d(sum_c l_c^T K r_c) / d l_a = -out[1 + a] / l_a
 * (the sign of the first-order entry points: one host assembly serves all three). */
int gpamd_kv_rbfgradgrad_plan(int n, int m, int d, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_floats);
int gpamd_kv_rbfgradgrad_partials_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                      float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
int64_t gpamd_kv_rbfgradgrad_grad_workspace_doubles(int n, int m, int d);
int gpamd_kv_rbfgradgrad_grad_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                                  const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- structured kernel interpolation (KISS-GP; the reference's gpytorch/utils/interpolation.py Interpolation.interpolate + the generic sparse
 * left_interp / left_t_interp of linear_operator it feeds): the products with the interpolation matrix W [n][M] of n points on a regular grid of
 * M = m_0 ... m_{d-1} nodes (d <= 3, every m_i >= 4, M <= 2^24; axis 0 slowest).  W is never stored: a point's 4^d cubic-convolution weights are
 * recomputed from its d coordinates.  X: the points, d floats per row, rows ldx floats apart (ldx >= d).  g0 / h / m: HOST arrays of d entries, the
 * first node, the spacing and the number of nodes of each axis; index arithmetic is float64, s = (x - g0) / h.  A point whose stencil base
 * floor(s) - 1 falls outside 0 .. m - 4 on an axis takes the clamped base and the one-hot weight of the nearest of the four nodes there (the
 * reference's boundary rule).  Probe-major vectors as everywhere: Out / V [t][ld >= n], U [t][ldg >= M].
 *   gpamd_ski_prepare_f32   keys[p] = sum_i b_i prod_{j > i} (m_j - 3), the cell of point p (b: the clamped stencil base).  The caller sorts the
 *                           keys (stable) into `perm` and counts them into cell_start [cells + 1], cells = prod (m_i - 3).
 *   gpamd_ski_interp_f32    Out = W U (replaces left_interp); perm: optional, lane i then handles point perm[i].
 *   gpamd_ski_interp_t_f32  U = W^T V (replaces left_t_interp) WITHOUT atomics: one node per lane sums the points of the <= 4^d cells whose stencil
 *                           holds it, in cell order, so the result is bitwise reproducible.  Cells with more than 256 points are summed in chunks
 *                           of 256 points first (chunk_off [cells + 1]: the first chunk of every cell; chunk_begin / chunk_end [nchunks]: each
 *                           chunk's range in the sorted order; workspace: gpamd_ski_workspace_floats(d, nchunks, t) floats).  nchunks == 0: no
 *                           such cell, the chunk arguments and the workspace may be NULL.
 *   gpamd_ski_interp_grad_f32  dX[p][a] = sum_c CA[c][p] sum_k (dw_pk / dx_a) GA[c][node_pk]  (+ the same sum over GB, CB): the gradient of a
 *                           bilinear form sum_c l_c^T (W_1 K_UU W_2^T) r_c with respect to the points of one cloud, from the grid vectors
 *                           G = K_UU W_other^T (other side's vectors) [t][ldg >= M] and the own side's vectors C [t][ldc >= n] as per-point
 *                           coefficients (the reference differentiates Interpolation.interpolate by autograd).  dw / dx_a: Keys' u' on axis a
 *                           (divided by h_a) times the plain weights on the other axes; an axis on which the point takes the boundary rule
 *                           contributes an exact zero.  GB and CB: a second pair read in the same pass (x1 is x2: both sides move the point),
 *                           or both NULL.  perm: optional, as gpamd_ski_interp_f32.  dX [n][lddx >= d] is written once, rows in the order of X;
 *                           weights and sums are float64, the order of the sums is fixed: bitwise reproducible.
 * GPAMD_EUNSUPPORTED: d outside 1..3, M > 2^24; GPAMD_EINVAL: a null pointer, m_i < 4, a non-positive spacing, a leading dimension or row stride
 * that is too small; GPAMD_EWORKSPACE: too few floats -- all before any launch. */
int gpamd_ski_prepare_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, int* keys, void* stream);
int gpamd_ski_interp_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm, const float* U,
                         int64_t ldg, int t, float* Out, int64_t ld, void* stream);
int gpamd_ski_interp_grad_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                              const float* GA, const float* CA, const float* GB, const float* CB, int64_t ldg, int64_t ldc, int t, float* dX,
                              int64_t lddx, void* stream);
int64_t gpamd_ski_workspace_floats(int d, int nchunks, int t);
int gpamd_ski_interp_t_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                           const int* cell_start, const int* chunk_off, const int* chunk_begin, const int* chunk_end, int nchunks, const float* V,
                           int64_t ldv, int t, float* U, int64_t ldg, float* workspace, int64_t workspace_floats, void* stream);

/* ---- ADDITIVE structured kernel interpolation: AdditiveStructureKernel over GridInterpolationKernel(num_dims=1)
 * (gpytorch/kernels/grid_interpolation_kernel.py:132-143, _compute_grid(last_dim_is_batch=True): every input column interpolated onto a
 * one-dimensional grid, and left_interp / left_t_interp of linear_operator under the resulting dimension batch, summed over it by
 * additive_structure_kernel.py:62-68).  One interpolation onto the CONCATENATION of d one-dimensional axes: W_add = [W_0 | .. | W_{d-1}] [n][M],
 * M = sum_q m_q, 4 d non-zeros per row; axis q occupies the nodes off_q .. off_q + m_q - 1, off_q = m_0 + .. + m_{q-1}.  The d axes are
 * INDEPENDENT (g0 / h / m: HOST arrays of d entries, 2 <= d <= 16); the per-axis rule is the one of gpamd_ski_*: float64 index arithmetic,
 * clamped base, one-hot boundary weights.  Arguments as the gpamd_ski_* twins, per axis and concatenated:
 *   gpamd_ski_add_prepare_f32   keys[q][p] (int [d][n]) = the clamped stencil base of point p on axis q.  The caller sorts every row (stable) and
 *                               lays the d sorted orders end to end: perm [d n] (point numbers; axis q at positions q n .. (q + 1) n - 1) and
 *                               cell_start [cells + 1], cells = sum_q (m_q - 3), cell coff_q + b with coff_q = sum_{r<q} (m_r - 3), as positions
 *                               in perm.
 *   gpamd_ski_add_interp_f32    Out = W_add U (replaces left_interp under the dimension batch and the sum over it): one lane per point, Out is
 *                               written once.  perm: optional [n], lane i then handles point perm[i].
 *   gpamd_ski_add_interp_t_f32  U = W_add^T V (replaces left_t_interp) WITHOUT atomics, all axes in one node launch: node j of axis q sums the
 *                               <= 4 cells j - o, o = 0..3 in that order, a cell's points in sorted order.  Cells with more than 256 points are
 *                               summed in chunks of 256 points first, the chunks of all axes in ONE launch (chunk_off [cells + 1], chunk_begin /
 *                               chunk_end [nchunks]: positions in perm; workspace: gpamd_ski_add_workspace_floats(d, nchunks, t) floats).  The
 *                               order of every sum is fixed (csrc/kv_ski_add.hpp): bitwise reproducible.
 * GPAMD_EUNSUPPORTED: d outside 2..16, M > 2^24; GPAMD_EINVAL: a null pointer, m_q < 4, a non-positive spacing, d n >= 2^31, a leading dimension
 * or row stride that is too small; GPAMD_EWORKSPACE: too few floats -- all on the host, before any launch. */
int gpamd_ski_add_prepare_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, int* keys, void* stream);
int gpamd_ski_add_interp_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                             const float* U, int64_t ldg, int t, float* Out, int64_t ld, void* stream);
int64_t gpamd_ski_add_workspace_floats(int d, int nchunks, int t);
int gpamd_ski_add_interp_t_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m, const int* perm,
                               const int* cell_start, const int* chunk_off, const int* chunk_begin, const int* chunk_end, int nchunks,
                               const float* V, int64_t ldv, int t, float* U, int64_t ldg, float* workspace, int64_t workspace_floats,
                               void* stream);

/* ---- batches of SMALL independent GPs (gpytorch/kernels/kernel.py:163-208 batch_shape; test/examples/test_batch_gp_regression.py).
 * Members below settings.max_cholesky_size are factorised, not iterated: what the member loop costs there is launches.  These two
 * entry points make the launch count independent of the batch size (blockIdx.z = member).  b members of n (resp. m) prepared points
 * each, stored back to back: X1p [b][n][dp], X2p [b][m][dp] (gpamd_prep_points_f32 per member, or the same arithmetic by the
 * caller); kparam [b] (RQ; NULL otherwise), scale [b] or NULL, dadd [b] or NULL (added on the diagonal i == j: K_hat in one pass).
 * out [b][n][ldo]:  out[g][i][j] = scale[g] k(x1_gi, x2_gj) + [i == j] dadd[g]   -- replaces the batched `Kernel.forward` +
 * `to_dense()` + `add_diagonal` of a batch-mode ExactGP (kernels/kernel.py:318-330, likelihoods/gaussian_likelihood.py:117-121). */
int gpamd_kernel_dense_batched_f32(int kind, const float* kparam, const float* X1p, int n, const float* X2p, int m, int dp, int b,
                                   const float* scale, const float* dadd, float* out, int64_t ldo, void* stream);
/* Batched bilinear derivative (the kernel backward of every member in one launch; functions/rbf_covariance.py:26-29,
 * matern_covariance.py:53-56): W [b][n][ldw] = d loss / d K_g;  G [b][2 + dp] (device doubles, zeroed here):
 * G[g][0] = sum W k,  G[g][1 + q] = sum W dk/ds (z_iq - z_jq)^2,  G[g][1 + dp] = sum W dk/dkparam at fixed s (RQ; 0 otherwise). */
int gpamd_kernel_grad_batched_f32(int kind, const float* kparam, const float* X1p, int n, const float* X2p, int m, int dp, int b,
                                  const float* W, int64_t ldw, double* G, void* stream);

/* ---- float64 (the reference honours float64 inputs).  Same conventions with double buffers.  The fused MFMA K*V
 * kernels are float32-only; in float64 K @ V is formed from dense row blocks of K generated by
 * gpamd_kernel_rows_f64 (rows == NULL: the block [row0, row0 + nrows); 1 <= nrows <= 65535, dp >= 1, ldo >= m, else GPAMD_EINVAL) times V with a library DGEMM by the caller,
 * then fed to the same device-resident mBCG through gpamd_cg64_reduce_q (S = 1). ---- */
int gpamd_prep_points_f64(int kind, double kparam, const double* X, int n, int d, int64_t ldx, const double* ls, int nls,
                          const double* shift, double* Xp, int dp, void* stream);
int gpamd_kernel_rows_f64(int kind, double kparam, const double* X1p, const int64_t* rows, int64_t row0, int nrows, const double* X2p, int m,
                          int dp, const double* scale, double* out, int64_t ldo, void* stream);
int gpamd_kernel_diag_f64(int kind, double kparam, const double* X1p, const double* X2p, int n, int dp, const double* scale, double* out,
                          void* stream);
/* Fused float64 K*V (kv_f64.hpp: float64 generation on the VALU, contraction on v_mfma_f64_16x16x4_f64 -- column groups of <= 4 columns on the
 * VALU: on gfx950 a float64 MFMA runs at the VALU's float64 rate and a 16-column tile would be mostly empty; d <= 16, else
 * GPAMD_EUNSUPPORTED and the caller uses the row-block path).  Same partial-slab convention as gpamd_kv_partials_f32:
 * P [S][t][ldo], to be summed / scaled by gpamd_kv_reduce_f64 or gpamd_cg64_reduce_q.  Replaces
 * KernelLinearOperator._matmul / LazyEvaluatedKernelTensor._matmul (lazy_evaluated_kernel_tensor.py:245-275) for
 * float64 models. */
int gpamd_kv_plan_f64(int n, int m, int dp, int t, int64_t ldo, int* S, int* jchunk, int64_t* workspace_doubles);
int gpamd_kv_partials_f64(int kind, double kparam, const double* X1p, int n, const double* X2p, int m, int dp, const double* Vt, int64_t ldv,
                          int t, double* P, int64_t ldo, int S, int jchunk, const int* done, void* stream);
/* Generic-path bilinear derivative, one row block (any dp; replaces, for float64 / d > 16, what gpamd_kv_grad_f32 does
 * fused; reference: the kernel backward, gpytorch/functions/rbf_covariance.py:26-29, matern_covariance.py:53-56).
 * W [nrows, ldw]: left^T right on entry, W * dk/ds on exit (s = squared prepared distance);
 * acc[0] += sum W * k and, for a family with a shape parameter (RQ), acc[1] += sum W * dk/dkparam at fixed s
 * (acc: TWO device doubles, zeroed by the caller). */
int gpamd_kernel_grad_block_f32(int kind, double kparam, const float* X1p, int64_t row0, int nrows, const float* X2p, int m, int dp, float* W,
                                int64_t ldw, double* acc, void* stream);
int gpamd_kernel_grad_block_f64(int kind, double kparam, const double* X1p, int64_t row0, int nrows, const double* X2p, int m, int dp, double* W,
                                int64_t ldw, double* acc, void* stream);
int gpamd_coldot_f64(const double* A, const double* B, int64_t ld, int n, int t, double* out, double* scratch, void* stream);
int gpamd_kv_reduce_f64(const double* P, int S, int64_t ldp, int t, int n, const double* scale, const double* dscale,
                        const double* dvec, const double* Vd, int64_t ldd, double* Out, int64_t ldo, const int* done,
                        void* stream);
typedef struct gpamd_cg64 gpamd_cg64_t;
int64_t gpamd_cg64_fscratch_elems(int t, int hist_len); /* layout / iscratch: as the float32 solver */
gpamd_cg64_t* gpamd_cg64_create(int n, int t, int64_t ld, double* X, double* R, double* D, double* Q, double* Z,
                                double* fscratch, int* iscratch, int hist_len, double eps, double stop_updating_after);
void gpamd_cg64_destroy(gpamd_cg64_t* h);
int gpamd_cg64_init(gpamd_cg64_t* h, const double* B, int64_t ldb, int have_precond, void* stream);
int gpamd_cg64_begin(gpamd_cg64_t* h, void* stream);
int gpamd_cg64_reduce_q(gpamd_cg64_t* h, const double* P, int S, int64_t ldp, const double* scale, const double* dscale,
                        const double* dvec, void* stream);
int gpamd_cg64_update_xr(gpamd_cg64_t* h, int k, void* stream);
int gpamd_cg64_update_d(gpamd_cg64_t* h, int k, void* stream);
int gpamd_cg64_stop(gpamd_cg64_t* h, int k, int min_iter, int tridiag_floor, double tol, void* stream);
int gpamd_cg64_finish(gpamd_cg64_t* h, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPAMD_H */
