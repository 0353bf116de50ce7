"""The covariance families of the fused kernels: codes, parameter blocks, torch restatements, and ONE ``Family`` record per kind (``FAMILIES``) with
the traits ``backend`` branches on -- it reads the record a ``PreparedPoints`` resolved once (``xp.family``).  A new family is one row here (and one
in csrc/api.hip ``ONE_KERNEL`` if it runs on a single kernel).  The switches tests assign (``FORCE_KV_FLAGS`` ...) live in ``backend``, not here."""
from __future__ import annotations

import ctypes as C
import math

import torch

KIND_IDS = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "rq": 4, "pp": 5, "prod": 6, "sm": 7, "add": 8, "ng": 9, "gibbs": 10}
# GPAMD_PS, the product-structure family.  Not a key of KIND_IDS: no entry point takes it as a `kind` (it has its own, which take base and d), and the
# table of kinds stays the eleven it was
PS_KIND_ID = 11
# GPAMD_HAMMING, the Hamming family over packed tokens: likewise its own entry points (width, 1 / alpha and beta as arguments), not a key of KIND_IDS
HAMMING_KIND_ID = 12
NU_TO_KIND = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def work_dtype(t: torch.Tensor) -> torch.dtype:
    """float64 tensors are computed in float64 (generic path), everything else in float32 (fused path)."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def pp_code(d: int, q: int) -> int:
    """Shape code 4 j + q of the piecewise-polynomial family for ``d`` input dimensions, j = floor(d / 2) + q + 1
    (``gpytorch/kernels/piecewise_polynomial_kernel.py:111``): what travels as ``kparam`` (csrc/common.hpp PPShape)."""
    if q not in (0, 1, 2, 3):
        raise ValueError("q expected to be 0, 1, 2 or 3")
    return 4 * (d // 2 + q + 1) + q


def pp_q2_c2(j):
    """The r^2 coefficient of P_2 as the reference EXECUTES it, (j + 4 j + 3) / 3 -- its docstring and Rasmussen & Williams eq. 4.21 say
    (j^2 + 4 j + 3) / 3.  The Python side's one place to switch when upstream changes it; the kernels' is ``pp_q2_c2`` in csrc/common.hpp."""
    return (j + 4 * j + 3) / 3.0


def pp_code_check(code) -> int:
    """The code as an integer, or ValueError: q in 0..3 and j >= q + 1 (the rule of csrc/host.hpp kparam_error)."""
    c = int(code)
    if c != code or c < 0 or (c >> 2) < (c & 3) + 1:
        raise ValueError("the piecewise-polynomial shape code must be 4 j + q with q in 0..3 and j >= q + 1")
    return c


PROD_FACTOR_KINDS = ("rbf", "matern12", "matern32", "matern52")   # the factors of the product family, by family id 0..3
PROD_MAX_FACTOR_DIM = 3     # columns per factor (csrc/kv_directp.hpp KDP_MAX_FACTOR_DIM)
_PROD_RULE = ("the product code must be K_A + 4 K_B + 16 D_A with K_A <= K_B <= 3 (family ids), not both RBF, 1 <= D_A <= 3, 1 <= d - D_A <= 3, "
              "and D_A <= d - D_A for equal families")


def prod_code(ka: int, kb: int, da: int) -> int:
    """Code K_A + 4 K_B + 16 D_A of the product family k_A(r_A) k_B(r_B): the factors' family ids (RBF 0, Matern-1/2 1, -3/2 2, -5/2 3) and the
    columns of the first factor; what travels as ``kparam`` (include/gpamd.h GPAMD_PROD).  Canonical order only: see ``prod_code_check``."""
    return prod_code_check(int(ka) + 4 * int(kb) + 16 * int(da))


def prod_decode(code: int):
    """(K_A, K_B, D_A) of a product code."""
    code = int(code)
    return code & 3, (code >> 2) & 3, code >> 4


def prod_code_check(code, d=None) -> int:
    """The code as an integer, or ValueError (the rule of csrc/host.hpp kparam_error; ``d`` = D_A + D_B where it is known)."""
    c = int(code)
    if c != code or not 0 <= c < 64:
        raise ValueError(_PROD_RULE)
    ka, kb, da = prod_decode(c)
    if ka > kb or kb == 0 or da < 1:
        raise ValueError(_PROD_RULE)
    if d is not None and (not 1 <= d - da <= PROD_MAX_FACTOR_DIM or (ka == kb and da > d - da)):
        raise ValueError(_PROD_RULE)
    return c


ADD_BASE_KINDS = PROD_FACTOR_KINDS   # the base families of the additive family, by family id 0..3
ADD_MIN_DIM, ADD_MAX_DIM = 2, 8     # input dimensions of the native additive family (csrc/kv_directadd.hpp KDA_MIN_DIM, KDA_MAX_DIM)
_ADD_RULE = "the additive family's code must be the base family's id -- 0 (RBF), 1, 2 or 3 (Matern 1/2, 3/2, 5/2) -- and d must be in 2..8"


def add_code(base_kind: str) -> int:
    """Code of the additive family k~ = (1/d) sum_q k'(|z_q - z'_q|) over the base family ``base_kind``: that family's id; what travels as ``kparam``
    (include/gpamd.h GPAMD_ADD)."""
    if base_kind not in ADD_BASE_KINDS:
        raise ValueError(_ADD_RULE)
    return KIND_IDS[base_kind]


def add_code_check(code, d=None) -> int:
    """The code as an integer, or ValueError (the rule of csrc/host.hpp kparam_error; ``d`` = the input dimensions where they are known)."""
    c = int(code)
    if c != code or not 0 <= c <= 3:
        raise ValueError(_ADD_RULE)
    if d is not None and not ADD_MIN_DIM <= d <= ADD_MAX_DIM:
        raise ValueError(_ADD_RULE)
    return c


NG_KSHIFT = 12              # the range shift of the split contraction, which rides in the weight block (csrc/kv_gramh.hpp KGH_KSHIFT)


def ng_cap(d: int, max_degree: int) -> int:
    """Degree cap of the native Newton-Girard kernel that serves ``max_degree`` at d dimensions = the length of its weight block and of the e_n sums
    its derivative kernel returns: min(d, 3) up to degree 3, d above (csrc/kv_directng.hpp ng_cap)."""
    return min(d, 3) if max_degree <= 3 else d


def ng_binomials(d: int, r: int, device=None, dtype=torch.float64) -> torch.Tensor:
    """C(d, n) for n = 1..r: e_n of d ones, the diagonal value of the n-th interaction order."""
    return torch.tensor([math.comb(d, n) for n in range(1, r + 1)], device=device, dtype=dtype)


class NGParams:
    """What a prepared Newton-Girard additive cloud carries in ``PreparedPoints.param``: the base family's id, d, max_degree R, the degree cap of the
    kernel, sigma in float64 (detached), S = sum_n sigma_n C(d, n) and the device block w_n = sigma_n / S * 2^12, zero above R (include/gpamd.h
    GPAMD_NG).  No host read of sigma."""

    def __init__(self, base: int, sigma, d: int):
        self.base, self.d = add_code_check(base, d), int(d)
        sig = sigma.detach().to(torch.float64).reshape(-1)
        self.r = int(sig.numel())
        if not 1 <= self.r <= self.d:
            raise ValueError(f"the Newton-Girard additive family takes max_degree in 1..d: got {self.r} outputscales at d = {d}")
        self.rc = ng_cap(self.d, self.r)
        self.sigma = sig
        self.s = (sig * ng_binomials(self.d, self.r, sig.device)).sum()
        self.what = torch.zeros(self.rc, device=sig.device, dtype=torch.float64)
        self.what[: self.r] = sig / self.s
        self.block = (self.what * float(1 << NG_KSHIFT)).to(torch.float32).contiguous()

    @property
    def base_kind(self) -> str:
        return ADD_BASE_KINDS[self.base]


def base_cov_prepared(kind: str, s: torch.Tensor) -> torch.Tensor:
    """RBF / Matern covariance of squared distances between PREPARED coordinates (the family constant folded in by ``prep_points``): 2^-s for the RBF,
    p(r) e^-r with r = sqrt(s) for Matern (csrc/common.hpp cov_factor_from_sq)."""
    if kind == "rbf":
        return torch.exp2(-s)
    r = s.sqrt()
    e = torch.exp(-r)
    return e if kind == "matern12" else ((1 + r) * e if kind == "matern32" else (1 + r + s / 3) * e)


def ng_esp(z: torch.Tensor, r: int):
    """[e_1 .. e_r] of the values along the LAST dimension of z, by the one-pass recursion with positive terms only (e_0 = 1; for every z_q, from the
    highest order down, e_n += z_q e_{n-1}) in the dtype of z: the arithmetic of csrc/kv_directng.hpp.  Autograd-visible (no in-place update)."""
    e = [torch.ones_like(z[..., 0])] + [None] * r
    for q in range(z.shape[-1]):
        zq = z[..., q]
        for n in range(min(q + 1, r), 0, -1):
            e[n] = zq * e[n - 1] if e[n] is None else e[n] + zq * e[n - 1]
    return e[1:]


def _cov_rows(xp1, xp2, rows, diag):
    """The prepared rows the torch restatements pair up: rows ``rows`` of xp1 (all when None) against every row of xp2, or with ``diag`` elementwise."""
    a = xp1.xp if rows is None else xp1.xp.index_select(0, rows)
    return (a, xp2.xp) if diag else (a.unsqueeze(1), xp2.xp.unsqueeze(0))


def ng_cov(xp1, xp2, rows=None, diag: bool = False) -> torch.Tensor:
    """k~ (the normalised Newton-Girard additive covariance, k / S) between prepared clouds, from the SAME prepared rows the fused kernels read, in float32 torch ops."""
    par = xp1.param
    a, b = _cov_rows(xp1, xp2, rows, diag)
    z = base_cov_prepared(par.base_kind, (a[..., : par.d] - b[..., : par.d]).square())
    w = par.what.to(z.dtype)
    e = ng_esp(z, par.r)
    out = w[0] * e[0]
    for n in range(1, par.r):
        out = out + w[n] * e[n]
    return out


PS_BASE_KINDS = ("matern12", "matern32", "matern52")   # the base families of the product-structure family (ids 1..3; csrc/kv_directps.hpp kps_base_ok)
_PS_RULE = ("the product-structure family's code must be the base family's id -- 1, 2 or 3 (Matern 1/2, 3/2, 5/2); a product of one-dimensional RBFs IS "
            "the 'rbf' family with per-dimension lengthscales -- and d must be in 2..8")


def ps_code(base_kind: str) -> int:
    """Code of the product-structure family k = prod_q k'(|z_q - z'_q|) over the Matern base family ``base_kind``: that family's id (include/gpamd.h
    GPAMD_PS)."""
    if base_kind not in PS_BASE_KINDS:
        raise ValueError(_PS_RULE)
    return KIND_IDS[base_kind]


class PSParams:
    """What a prepared product-structure cloud carries in ``PreparedPoints.param``: the base family's id and d.  The family has no parameter block."""

    def __init__(self, base, d: int):
        b = int(base)
        if b != base or not 1 <= b <= 3 or not ADD_MIN_DIM <= int(d) <= ADD_MAX_DIM:
            raise ValueError(_PS_RULE)
        self.base, self.d = b, int(d)

    @property
    def base_kind(self) -> str:
        return ADD_BASE_KINDS[self.base]


def ps_tree(vs, op):
    """vs[0] op vs[1] op .. pairwise, (v0 op v1) op (v2 op v3) ..: the order of csrc/kv_directps.hpp kps_tree."""
    vs, s = list(vs), 1
    while s < len(vs):
        for j in range(0, len(vs) - s, 2 * s):
            vs[j] = op(vs[j], vs[j + s])
        s *= 2
    return vs[0]


def ps_cov(xp1, xp2, rows=None, diag: bool = False) -> torch.Tensor:
    """The product-structure (tensor-product Matern) covariance between prepared clouds, from the SAME prepared rows the fused kernels read, in float32
    torch ops and in their arithmetic: k = exp2(-log2(e) sum_q r_q) prod_q p(r_q), r_q = |z_q - z'_q|, p = 1, 1 + r, 1 + r + r^2 / 3, sum and product
    pairwise (``ps_tree``).  Identical rows give r_q = 0 and an exact 1: the self-diagonal holds exact ones."""
    par = xp1.param
    a, b = _cov_rows(xp1, xp2, rows, diag)
    r = (a[..., : par.d] - b[..., : par.d]).abs().unbind(-1)
    k = torch.exp2(-1.4426950408889634 * ps_tree(r, torch.add))
    if par.base == 1:
        return k
    p = [1.0 + rq for rq in r]
    if par.base == 3:
        p = [pq + (rq * rq) * (1.0 / 3.0) for pq, rq in zip(p, r)]
    return k * ps_tree(p, torch.mul)


SM_MAX_DIM = 3              # input dimensions of the native spectral-mixture family (csrc/kv_directsm.hpp KSM_MAX_DIM)


def sm_max_mixtures(d: int) -> int:
    """Mixtures Q the native spectral-mixture kernels exist for at d input dimensions (csrc/kv_directsm.hpp ksm_max_q)."""
    return 8 if d == 1 else 4


def sm_envelope_ok(q: int, d: int) -> bool:
    return 1 <= d <= SM_MAX_DIM and 1 <= q <= sm_max_mixtures(d)


def sm_theta(weights, means, scales):
    """theta = [w | mu | sigma], the ONE tensor in which the three spectral-mixture parameter tensors ([Q], [Q, 1, d], [Q, 1, d]) travel through the
    learnable-parameter slot of the autograd Functions (differentiable: a concatenation of views)."""
    return torch.cat([weights.reshape(-1), means.reshape(-1), scales.reshape(-1)])


def sm_theta_split(theta, d: int):
    """(w [Q], mu [Q, d], sigma [Q, d]) of theta = [w | mu | sigma] at d input dimensions."""
    q, rem = divmod(theta.numel(), 1 + 2 * d)
    if rem or q < 1:
        raise ValueError(f"a spectral-mixture parameter vector at d = {d} holds Q (1 + 2 d) values, got {theta.numel()}")
    return theta[:q], theta[q : q + q * d].reshape(q, d), theta[q + q * d :].reshape(q, d)


class SMParams:
    """What a prepared spectral-mixture cloud carries in ``PreparedPoints.param``: Q, d, the parameters in float64 (detached) and the device block
    na[q d + j] = -2 pi^2 sigma_qj^2 log2(e) of the kernels (include/gpamd.h GPAMD_SM)."""

    def __init__(self, theta, d: int):
        w, mu, sigma = (t.detach().to(torch.float64) for t in sm_theta_split(theta, d))
        self.q, self.d = int(w.numel()), int(d)
        self.w, self.mu, self.sigma = w, mu, sigma
        self.wsum = w.sum()
        self.what = w / self.wsum
        self.block = (-2.0 * math.pi ** 2 * math.log2(math.e) * sigma * sigma).to(torch.float32).reshape(-1).contiguous()

    @property
    def width(self) -> int:
        return self.d + 2 * self.q * self.d


def sm_prep(x: torch.Tensor, shift, par: SMParams) -> torch.Tensor:
    """The prepared rows of the spectral-mixture family, float32 [n, round_up(d + 2 Q d, 4)]:
    [x - shift | sqrt(w^_q) cos(2 pi phi), sqrt(w^_q) sin(2 pi phi) at columns d + 2 (q d + j), + 1 | zeros],  phi = frac(x_j mu_qj) IN FLOAT64, reduced to
    [0, 1) before the cosine / sine and before the cast (a float32 phase loses 1e-2 of the cosine at |x| = 1000, mu = 5)."""
    n, d = x.shape
    x64 = x.detach().to(torch.float64)
    phi = x64.unsqueeze(1) * par.mu.unsqueeze(0)                     # [n, Q, d]
    phi = (phi - torch.floor(phi)) * (2.0 * math.pi)
    amp = par.what.sqrt().reshape(1, -1, 1)
    feat = torch.stack([amp * torch.cos(phi), amp * torch.sin(phi)], dim=-1).reshape(n, 2 * par.q * d)   # (q, j, cos | sin)
    xc = x64 if shift is None else x64 - shift.detach().to(device=x.device, dtype=torch.float64).reshape(1, d)
    xp = torch.zeros(n, round_up(par.width, 4), device=x.device, dtype=torch.float32)
    xp[:, :d] = xc
    xp[:, d : par.width] = feat
    return xp


def sm_cov(xp1, xp2, rows=None, diag: bool = False) -> torch.Tensor:
    """k~ (the normalised spectral-mixture covariance, k / Wsum^d) between prepared clouds, from the SAME prepared rows the fused kernels read, in float32 torch ops."""
    par = xp1.param
    a, b = _cov_rows(xp1, xp2, rows, diag)
    d, q = par.d, par.q
    tau2 = (a[..., :d] - b[..., :d]).square().unsqueeze(-2)                        # [..., 1, d]
    fa = a[..., d : par.width].reshape(*a.shape[:-1], q, d, 2)
    fb = b[..., d : par.width].reshape(*b.shape[:-1], q, d, 2)
    e = torch.exp2(tau2 * par.block.reshape(q, d))
    return (e * (fa * fb).sum(-1)).sum(-2).prod(-1)


GIBBS_MAX_DIM = 6           # input dimensions of the native Gibbs family (csrc/kv_directgibbs.hpp KGB_MAX_DIM)
# The exponent of the Gibbs prefactor (2 l l' / (l^2 + l'^2)) as the reference EXECUTES it (``gpytorch/kernels/gibbs_kernel.py:81``): 1/2 for every d,
# where Gibbs / Paciorek-Schervish have d / 2 -- for d >= 2 with a varying l the matrix is not positive definite in general.  The Python side's one place
# to switch when upstream changes it; the kernels' is ``GIBBS_PREFACTOR_EXPONENT`` in csrc/kv_directgibbs.hpp.
GIBBS_PREFACTOR_EXPONENT = 0.5


def gibbs_width(d: int) -> int:
    """Width of a prepared Gibbs row at d input dimensions: a, q and the d coordinates padded to 4 (d <= 2) or 8 (d <= 6) columns."""
    return round_up(2 + d, 4)


class GibbsParams:
    """What a prepared Gibbs cloud carries in ``PreparedPoints.param``: d and the prepared width.  Every parameter of the family is per point, in the rows."""

    def __init__(self, d: int):
        self.d, self.width = int(d), gibbs_width(d)


def gibbs_prep(z: torch.Tensor, shift) -> torch.Tensor:
    """The prepared rows of the Gibbs family from the AUGMENTED cloud z = [x | l] ([n, d + 1], l = lengthscale_fn(x) > 0), float32 [n, 4 or 8]:
        [ a = l^2 | q = (sqrt(2) l)^GIBBS_PREFACTOR_EXPONENT = 2^(1/4) sqrt(l) | x - shift (d columns) | zeros ]
    with float64 intermediates (include/gpamd.h GPAMD_GIBBS is the ABI's statement of the same layout; csrc/kv_directgibbs.hpp reads it).  a and q come
    first and the padding is zero, so the kernels do not know d.  ``shift``: d + 1 values (its last one, for the l column, is not used) or None.  A
    non-positive or non-finite l gives NaN rows, as the reference gives NaN values: no host read, no check."""
    n, d = z.shape[0], z.shape[1] - 1
    z64 = z.detach().to(torch.float64)
    l = z64[:, d]
    xc = z64[:, :d] if shift is None else z64[:, :d] - shift.detach().to(device=z.device, dtype=torch.float64).reshape(-1)[:d]
    xp = torch.zeros(n, gibbs_width(d), device=z.device, dtype=torch.float32)
    xp[:, 0] = l * l
    xp[:, 1] = (math.sqrt(2.0) * l) ** GIBBS_PREFACTOR_EXPONENT
    xp[:, 2 : 2 + d] = xc
    return xp


def gibbs_cov(xp1, xp2, rows=None, diag: bool = False) -> torch.Tensor:
    """The Gibbs covariance between prepared clouds, from the SAME prepared rows the fused kernels read, in float32 torch ops and in their arithmetic:
    k = q_i q_j u exp2(-log2(e) s u^2), u = rsqrt(a_i + a_j), s over every column behind the first two (the padding adds zero)."""
    if diag and xp2 is xp1 and rows is None:   # k(x, x) = 1 exactly (q^2 u = 1 holds to rounding only)
        return torch.ones(xp1.n, device=xp1.xp.device, dtype=torch.float32)
    a, b = _cov_rows(xp1, xp2, rows, diag)
    s = (a[..., 2:] - b[..., 2:]).square().sum(-1)
    u = torch.rsqrt(a[..., 0] + b[..., 0])
    return (a[..., 1] * b[..., 1]) * u * torch.exp2(-1.4426950408889634 * s * (u * u))


HAMMING_MAX_POSITIONS = 128   # sequence length T of the native Hamming family (csrc/kv_directham.hpp KHM_MAX_POSITIONS)
HAMMING_MAX_VOCAB = 126       # vocabulary size V: a position is stored as the byte token + 1 in 1..127
HAMMING_WIDTHS = (4, 8, 16, 32)   # instantiated widths of a prepared row in dwords (csrc/kv_directham.hpp khm_width_ok): T <= 16, 32, 64, 128


def hamming_width(t: int) -> int:
    """Width in dwords of a prepared Hamming row of T positions: the first instantiated width with 4 W >= T."""
    for w in HAMMING_WIDTHS:
        if t <= 4 * w:
            return w
    raise ValueError(f"the native Hamming family takes sequences of at most {HAMMING_MAX_POSITIONS} positions: got {t}")


def hamming_prep(x: torch.Tensor, vocab_size: int):
    """The prepared rows of the Hamming family from one-hot encoded sequences x, float32 [n, T V], and whether x IS one-hot:
        (rows, valid)   rows: an int8 tensor [n, 4 W] viewed as float32 [n, W] (what ``PreparedPoints`` carries), W = ``hamming_width(T)``
                        valid: a 0-d bool tensor on x's device -- every position of every row has one entry equal to 1 and V - 1 equal to 0
    Position p of a row is the byte ``argmax over its V columns + 1`` at byte p of the row (four positions per dword); the bytes behind position T - 1
    are 1.  Bytes lie in 1..127 (V <= 126), so every dword is a normal, finite float bit pattern whatever copies it, and the kernels count the
    differing positions of two dwords as popcount(((a ^ b) + 0x7f7f7f7f) & 0x80808080) (include/gpamd.h GPAMD_HAMMING is the ABI's statement of the
    same layout; csrc/kv_directham.hpp reads it).  Equal padding contributes nothing to a distance.  Nothing is read back on the host here: a caller
    that cannot vouch for its input reads ``valid`` (``kernels.HammingIMQKernel`` does, once per cloud) -- for an input that is not one-hot the rows
    describe the argmax sequence, not x."""
    v = int(vocab_size)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("the Hamming family takes one float32 [n, T V] cloud of one-hot encoded sequences (no batches)")
    if not 1 <= v <= HAMMING_MAX_VOCAB or x.shape[1] == 0 or x.shape[1] % v:
        raise ValueError(f"the native Hamming family takes a vocabulary of 1..{HAMMING_MAX_VOCAB} letters that divides the input width: got V = {v}, width {x.shape[1]}")
    n, t = x.shape[0], x.shape[1] // v
    w = hamming_width(t)
    x3 = x.detach().reshape(n, t, v)
    packed = torch.ones(n, 4 * w, device=x.device, dtype=torch.int8)
    packed[:, :t] = (x3.argmax(-1) + 1).to(torch.int8)
    valid = (((x3 == 1).sum(-1) == 1) & ((x3 != 0).sum(-1) == 1)).all()
    return packed.view(torch.float32), valid


class HammingParams:
    """What a prepared Hamming cloud carries in ``PreparedPoints.param``: T, V, the prepared width W, alpha and beta detached in float64, and
    ``inv_alpha`` = 1 / alpha and ``beta_f`` as the kernels take them -- by value, rounded to float32 (one host read per evaluation, the precedent
    being RQ's alpha)."""

    def __init__(self, t: int, vocab_size: int, alpha, beta):
        self.t, self.v, self.width = int(t), int(vocab_size), hamming_width(int(t))
        self.alpha = torch.as_tensor(alpha).detach().to(torch.float64).reshape(())
        self.beta = torch.as_tensor(beta).detach().to(torch.float64).reshape(())
        a, b = float(self.alpha), float(self.beta)
        if not (a > 0.0 and b > 0.0 and math.isfinite(a) and math.isfinite(b)):
            raise ValueError("the Hamming family needs positive, finite alpha and beta")
        self.inv_alpha = float(torch.tensor(1.0 / a, dtype=torch.float32))
        self.beta_f = float(torch.tensor(b, dtype=torch.float32))


def hamming_cov(xp1, xp2, rows=None, diag: bool = False) -> torch.Tensor:
    """k~ = (1 + c / alpha)^(-beta) in (0, 1] (the Hamming covariance without its constant k0 = ((1 + alpha) / alpha)^beta, which rides in the
    operator's outputscale slot) between prepared clouds, from the SAME prepared rows the fused kernels read -- bytes unpacked, c = the number of
    differing bytes -- in float32 torch ops and in the kernels' arithmetic: s = float(c) (1 / alpha), k~ = exp2(-beta log2(1 + s)).  c = 0 gives an
    exact 1: log2(1) = 0."""
    par = xp1.param
    if diag and xp2 is xp1 and rows is None:
        return torch.ones(xp1.n, device=xp1.xp.device, dtype=torch.float32)
    a, b = _cov_rows(xp1, xp2, rows, diag)
    a, b = a.view(torch.int8), b.view(torch.int8)
    if diag:
        c = (a != b).sum(-1, dtype=torch.int32)
    else:   # row blocks, so that the byte comparison (rows x m x 4 W) stays within 64 MiB whatever the size of the block asked for
        step = max(1, (1 << 26) // max(1, b.shape[1] * b.shape[2]))
        c = torch.cat([(a[r0 : r0 + step] != b).sum(-1, dtype=torch.int32) for r0 in range(0, a.shape[0], step)]) if a.shape[0] else \
            torch.zeros(0, b.shape[1], device=b.device, dtype=torch.int32)
    s = c.to(torch.float32) * par.inv_alpha
    return torch.exp2(-par.beta_f * torch.log2(1.0 + s))


def cusp_at_origin(xp) -> bool:
    """k is not differentiable in the SQUARED distance at zero (Matern nu = 1/2; the piecewise polynomial with q = 0): the 1e-6 error of the
    quadratic expansion would show as 1e-3 in r, so these stay on the direct-difference kernels, forward and backward."""
    return xp.kind == "matern12" or (xp.kind == "pp" and (int(xp.param) & 3) == 0)


# d s / d l factors: s = sum_q z_q^2-differences with z = coef * x / l  =>  ds_q/dl_q = -2 s_q / l_q
RBF_PREP_COEF = math.sqrt(0.5 * 1.4426950408889634)


def prep_coef(kind: str) -> float:
    """z = coef * (x - shift) / lengthscale (prep_points): sqrt(log2(e)/2) for RBF, sqrt(2 nu) for Matern."""
    return {"rbf": RBF_PREP_COEF, "matern12": 1.0, "matern32": math.sqrt(3.0), "matern52": math.sqrt(5.0), "pp": 1.0}[kind]


def prod_prep_coefs(code: int, d: int) -> list:
    """The product family's factor PER DIMENSION: the first factor's constant for its D_A columns, the second's for the other d - D_A."""
    ka, kb, da = prod_decode(prod_code_check(code, d))
    return [prep_coef(PROD_FACTOR_KINDS[ka])] * da + [prep_coef(PROD_FACTOR_KINDS[kb])] * (d - da)


# ---- the records.  ``prepare(x, shift, param)`` -> (param as the prepared cloud carries it, (kind, kparam) of the library's preparation kernel, rows
# prepared here in torch or None), after validating the parameter against the cloud; None: a family without parameter
def _f32_cloud(x, name: str, batches: bool = False):
    if work_dtype(x) != torch.float32:
        raise ValueError(f"the {name} family is float32 only")
    if not batches and x.dim() != 2:
        raise ValueError(f"the {name} family takes one [n, d] cloud (no batches)")


def _rq_alpha(param, d):
    param = float(param)
    if not param > 0.0:
        raise ValueError("the rational-quadratic shape parameter alpha must be positive")
    return param


def _kparam_family(kind, needs, check, f32=None, batches=True):
    """``prepare`` of a family whose parameter is a number that travels as kparam: ``check(param, d)`` returns it validated."""
    def prepare(x, shift, param):
        if param is None:
            raise ValueError(f"the {needs}")
        if f32 is not None:
            _f32_cloud(x, f32, batches)
        param = check(param, x.shape[-1])   # (additive: the padding columns of its prepared rows hold NaN, csrc/common.hpp)
        return param, (KIND_IDS[kind], param), None
    return prepare


def _prepare_ng(x, shift, param):
    # the parameter is (base family id, sigma) (or an NGParams built from them), not a number; the rows are the BASE family's (zero padding)
    if param is None:
        raise ValueError("the Newton-Girard additive family needs (base family id, outputscales)")
    _f32_cloud(x, "Newton-Girard additive")
    par = param if isinstance(param, NGParams) else NGParams(param[0], param[1], x.shape[-1])
    if par.d != x.shape[-1]:
        raise ValueError(f"Newton-Girard parameters for d = {par.d} with points of d = {x.shape[-1]}")
    return par, (par.base, 0.0), None


def _prepare_ps(x, shift, param):
    # the parameter is the base family's id 1..3 (or a PSParams built from it); the rows are the BASE family's (zero padding: d travels as an argument)
    if param is None:
        raise ValueError("the product-structure family needs its code: the base family's id 1..3 (Matern 1/2, 3/2, 5/2)")
    _f32_cloud(x, "product-structure")
    par = param if isinstance(param, PSParams) else PSParams(param, x.shape[-1])
    if par.d != x.shape[-1]:
        raise ValueError(f"product-structure parameters for d = {par.d} with points of d = {x.shape[-1]}")
    return par, (par.base, 0.0), None


def _prepare_sm(x, shift, param):
    # the parameter is theta = [w | mu | sigma] (or an SMParams built from it), not a number; the rows are prepared here, in float64 torch ops
    # (the family has no lengthscale: the slot carries ones and is not read -- no host read of any parameter on this path)
    if param is None:
        raise ValueError("the spectral-mixture family needs its parameters theta = [w | mu | sigma]")
    _f32_cloud(x, "spectral-mixture", batches=True)
    par = param if isinstance(param, SMParams) else SMParams(param, x.shape[-1])
    if par.d != x.shape[-1] or not sm_envelope_ok(par.q, par.d):
        raise ValueError(f"the native spectral-mixture family takes d in 1..3 and Q <= 8 (d = 1) or 4 (d = 2, 3): got Q = {par.q}, d = {x.shape[-1]}")
    _f32_cloud(x, "spectral-mixture")
    return par, None, sm_prep(x, shift, par)


def _prepare_gibbs(x, shift, param):
    # x is the augmented cloud [x | l]: the rows are prepared here, in float64 torch ops; the family has no parameter of its own (``param`` is ignored)
    _f32_cloud(x, "Gibbs")
    d = x.shape[-1] - 1
    if not 1 <= d <= GIBBS_MAX_DIM:
        raise ValueError(f"the native Gibbs family takes augmented points [x | l] with 1 <= d <= {GIBBS_MAX_DIM}: got {x.shape[-1]} columns")
    return GibbsParams(d), None, gibbs_prep(x, shift)


def _prepare_hamming(x, shift, param):
    # x is the one-hot cloud [n, T V]; the parameter is (vocabulary size, theta = [alpha, beta]) (or a HammingParams built from them); the rows are
    # prepared here in torch ops (``shift`` is not used: tokens have no origin).  Whether x is one-hot is the caller's to check (``hamming_prep``)
    if param is None:
        raise ValueError("the Hamming family needs (vocabulary size, [alpha, beta])")
    _f32_cloud(x, "Hamming")
    if isinstance(param, HammingParams):
        par = param
    else:
        v, theta = int(param[0]), torch.as_tensor(param[1]).reshape(-1)
        if v < 1 or x.shape[-1] % v:
            raise ValueError(f"the Hamming family takes an input width that is a multiple of the vocabulary size: got width {x.shape[-1]}, V = {v}")
        par = HammingParams(x.shape[-1] // v, v, theta[0], theta[1])
    if par.t * par.v != x.shape[-1]:
        raise ValueError(f"Hamming parameters for T V = {par.t * par.v} with points of width {x.shape[-1]}")
    return par, None, hamming_prep(x, par.v)[0]


def _spec_number(spec):
    """``spec_param`` (what ``prep_points`` takes as ``param`` for a ``functions.KernelSpec``) of a family whose parameter is a number: the shape
    code, or the shape parameter as a Python float for the C ABI (one host read per evaluation), or None."""
    if spec.code is not None:
        return spec.code
    return None if spec.param is None else float(spec.param.detach().reshape(-1)[0])


class Family:
    """One covariance family as the host code sees it.  ``one_kernel``: direct differences + split contraction at every column count -- no Gram
    policy, no tile culling, always ``KV_SPLIT`` (``FORCE_KV_FLAGS`` and ``settings.split_contraction`` have nothing to choose between).
    ``has_f64``: the fused float64 kernel knows the family;  ``widenable``: its float32 prepared rows may be widened for the float64 corrections.
    ``plan_kind``: the kind ``gpamd_kv_plan`` is asked with, ``plan_dims(d)``: the dimension count it is asked with.  ``stackable``: batched members can be stacked into one kernel.  ``cov``: the point-wise
    covariance as a torch expression on prepared rows, None where the library has native kernels.  ``grad_param``: the family's name in ``kv_grad``
    where its derivative needs the entry point that carries kparam.  ``coef``: the preparation factor of a prepared cloud (``backend.prep_coef_of``;
    None: ``prep_coef`` of the kind), or the text of the family's refusal.  ``launch(L, x1, X1, n, X2, m, *tail)``: one K*V launch group through the
    family's OWN entry point (it travels with a parameter block; None: gpamd_kv_partials_f32)."""
    one_kernel, has_f64, widenable, stackable = False, True, True, True
    prepare = cov = launch = coef = grad_param = None
    spec_param = staticmethod(_spec_number)
    plan_dims = staticmethod(lambda d: d)

    def __init__(self, name, **traits):
        self.name, self.id, self.plan_kind = name, KIND_IDS.get(name), name
        self.__dict__.update(traits)


_ONE = dict(one_kernel=True, has_f64=False)
FAMILIES = {f.name: f for f in (
    Family("rbf"), Family("matern12"), Family("matern32"), Family("matern52"),
    Family("rq", prepare=_kparam_family("rq", "rational-quadratic family needs its shape parameter alpha", _rq_alpha),
           coef=lambda xp: 1.0 / math.sqrt(2.0 * xp.param)),
    Family("pp", prepare=_kparam_family("pp", "piecewise-polynomial family needs its shape code 4 j + q", lambda code, d: pp_code_check(code)),
           grad_param="piecewise polynomial"),
    Family("prod", prepare=_kparam_family("prod", "product family needs its code K_A + 4 K_B + 16 D_A", prod_code_check, f32="product"), **_ONE,
           coef="the product family has one preparation factor per column group: backend.prod_prep_coefs", stackable=False, grad_param="product"),
    Family("sm", prepare=_prepare_sm, **_ONE, coef="the spectral-mixture family has no lengthscale and no preparation factor",
           widenable=False, cov=sm_cov, spec_param=lambda spec: spec.param.detach(),   # (x1.d: the prepared width)
           launch=lambda L, x1, *a: L.gpamd_kv_sm_partials_f32(_ptr(x1.param.block), x1.param.q, x1.param.d, *a[:4], x1.d, *a[4:])),
    Family("add", prepare=_kparam_family("add", "additive family needs its code: the base family's id 0..3", add_code_check, "additive", False), **_ONE,
           coef=lambda xp: prep_coef(ADD_BASE_KINDS[int(xp.param)]), widenable=False, stackable=False, grad_param="additive"),
    # (both additive families scale every column as the base family prescribes; this one is planned as the additive family of the same d: one kernel
    #  body, tile geometry and launch bounds; its parameter is (base family id, detached outputscales), a device block for the kernels -- no host read)
    Family("ng", prepare=_prepare_ng, **_ONE, coef=lambda xp: prep_coef(xp.param.base_kind), widenable=False, plan_kind="add", stackable=False,
           cov=ng_cov, spec_param=lambda spec: (spec.code, spec.param.detach()),
           launch=lambda L, x1, *a: L.gpamd_kv_ng_partials_f32(_ptr(x1.param.block), x1.param.base, x1.param.d, x1.param.r, *a)),
    # (the tensor-product Matern family: the base family's rows, planned as the additive family of the same d like "ng"; no block -- base and d are arguments)
    Family("ps", id=PS_KIND_ID, prepare=_prepare_ps, **_ONE, coef=lambda xp: prep_coef(xp.param.base_kind), widenable=False, plan_kind="add", stackable=False,
           cov=ps_cov, spec_param=lambda spec: spec.code,
           launch=lambda L, x1, *a: L.gpamd_kv_ps_partials_f32(x1.param.base, x1.param.d, *a)),
    # (the points are the augmented cloud [x | l(x)]: every parameter is per point, in the prepared rows; kind 10 through the shared entry points with
    #  d = the prepared width (x1.d), no kparam, no centres, GPAMD_KV_SPLIT (8))
    Family("gibbs", prepare=_prepare_gibbs, **_ONE, coef="the Gibbs family has per-point lengthscales and no preparation factor", widenable=False,
           stackable=False, cov=gibbs_cov, spec_param=lambda spec: None,
           launch=lambda L, x1, *a: L.gpamd_kv_partials_f32(KIND_IDS["gibbs"], 0.0, *a[:4], x1.d, None, *a[4:11], 8, *a[11:])),
    # (sequences as packed tokens, one byte per position: the rows are prepared here and are not numbers -- no lengthscale, no preparation factor, no
    #  centring.  Planned as the Gibbs family at width min(W, 8): one kernel body, tile geometry, launch bounds and row-tile rule, and neither the split
    #  nor the workspace depends on the width.  Its parameter is (vocabulary size, [alpha, beta]); 1 / alpha and beta are arguments of its entry points)
    Family("hamming", id=HAMMING_KIND_ID, prepare=_prepare_hamming, **_ONE, coef="the Hamming family has no lengthscale and no preparation factor",
           widenable=False, plan_kind="gibbs", plan_dims=lambda d: min(d, 8), stackable=False, cov=hamming_cov,
           spec_param=lambda spec: (spec.code, spec.param.detach()),
           launch=lambda L, x1, *a: L.gpamd_kv_hamming_partials_f32(x1.param.width, x1.param.inv_alpha, x1.param.beta_f, *a)),
)}
