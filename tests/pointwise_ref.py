"""float64 torch restatement of the POINT-WISE operations of the library -- point preparation, the covariance of two prepared rows, its derivatives
and the two derivative reductions -- the oracle of test_gpu_pointwise.py.  Written from the formulas of include/gpamd.h and the "Covariance families"
comment of csrc/common.hpp; it calls neither ``gpytorch_amd.families`` nor a kernel.  test_pointwise_ref_cpu.py ties it to the older restatements
(oracle/kernels.py, tests/piecewise_ref.py, tests/product_ref.py, tests/additive_ref.py) and its derivatives to autograd.

Prepared coordinates (z = (x - shift) coef / lengthscale) and the covariance as a function of s = |z - z'|^2, r = sqrt(s):
    rbf       coef sqrt(log2(e) / 2)        k = 2^-s
    matern12  coef 1                        k = e^-r
    matern32  coef sqrt(3)                  k = (1 + r) e^-r
    matern52  coef sqrt(5)                  k = (1 + r + s / 3) e^-r
    rq        coef 1 / sqrt(2 alpha)        k = (1 + s)^-alpha                                   param = alpha
    pp        coef 1                        k = max(1 - r, 0)^(j + q) P_q(r)                     param = the code 4 j + q
    prod      coef of K_A, of K_B from D_A  k = k_A(s over columns < D_A) k_B(s over the rest)   param = the code K_A + 4 K_B + 16 D_A
    add       coef of the base family       k = mean over the non-NaN columns of k'((z_q - z'_q)^2)   param = the base family's id; NaN padding
"""
import math

import torch

F64 = torch.float64
KIND_ID = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "rq": 4, "pp": 5, "prod": 6, "add": 8}   # include/gpamd.h GPAMD_*
BASE = ("rbf", "matern12", "matern32", "matern52")   # by family id 0..3
LN2 = math.log(2.0)


def prod_shape(code):
    code = int(code)
    return code & 3, (code >> 2) & 3, code >> 4   # K_A, K_B, D_A


def pp_shape(code):
    """(e, c1, c2, c3, b0, b1, b2, sing) of the code 4 j + q: k = u^e (1 + c1 r + c2 r^2 + c3 r^3), dk/ds = u^(e-1) (b0 + b1 r + b2 r^2 + sing / r) / 2.
    The r^2 coefficient of q = 2 is the one the reference executes, (j + 4 j + 3) / 3 (csrc/common.hpp pp_q2_c2)."""
    code = int(code)
    q, j = code & 3, float(code >> 2)
    e = j + q
    c1 = e if q >= 1 else 0.0
    c2 = (j + 4 * j + 3) / 3 if q == 2 else ((6 * j * j + 36 * j + 45) / 15 if q == 3 else 0.0)
    c3 = (j ** 3 + 9 * j * j + 23 * j + 15) / 15 if q == 3 else 0.0
    return e, c1, c2, c3, 2 * c2 - (e + 1) * c1, 3 * c3 - (e + 2) * c2, -(e + 3) * c3, (-e if q == 0 else 0.0)


def coef(kind, param=0.0, dtype=F64):
    """The constant of point preparation, evaluated in ``dtype`` the way the host evaluates it (one sqrt, one product or quotient)."""
    if kind == "rbf":
        return float((torch.tensor(1.4426950408889634, dtype=dtype) * 0.5).sqrt())
    if kind in ("matern12", "pp"):
        return 1.0
    if kind in ("matern32", "matern52"):
        return float(torch.tensor(3.0 if kind == "matern32" else 5.0, dtype=dtype).sqrt())
    if kind == "rq":
        return float(1.0 / (torch.tensor(2.0, dtype=dtype) * torch.tensor(param, dtype=dtype)).sqrt())
    raise ValueError(kind)


def prep(kind, x, ls, shift, param, dp, coef_dtype=F64):
    """Prepared rows [n, dp] in float64 of x [n, d]; ls: 1 or d lengthscales; shift: d-vector or None; the columns from d on are zero (``add``: NaN).
    ``prod``: columns < D_A take the constant of K_A, the others that of K_B; ``add``: every column the base family's."""
    x = torch.as_tensor(x).double()
    n, d = x.shape
    ls = torch.as_tensor(ls).double().reshape(-1)
    ls = ls.expand(d) if ls.numel() == 1 else ls
    if kind == "prod":
        ka, kb, da = prod_shape(param)
        c = torch.tensor([coef(BASE[ka], 0.0, coef_dtype) if k < da else coef(BASE[kb], 0.0, coef_dtype) for k in range(d)], dtype=F64)
    else:
        c = torch.full((d,), coef(BASE[int(param)] if kind == "add" else kind, param, coef_dtype), dtype=F64)
    sh = torch.zeros(d, dtype=F64) if shift is None else torch.as_tensor(shift).double().reshape(-1)
    out = torch.full((n, dp), float("nan") if kind == "add" else 0.0, dtype=F64)
    out[:, :d] = (x - sh) * (c / ls)
    return out


def _safe_sqrt(s):
    pos = s > 0
    return torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


def cov_s(kind, s, param=0.0):
    """k as a function of the squared prepared distance (the six single-parameter families), elementwise."""
    if kind == "rbf":
        return torch.exp2(-s)
    if kind == "rq":
        return (1 + s).pow(-param)
    r = _safe_sqrt(s)
    if kind == "pp":
        e, c1, c2, c3 = pp_shape(param)[:4]
        u = (1 - r).clamp_min(0)
        return u.pow(e) * (1 + c1 * r + c2 * r * r + c3 * r ** 3)
    ex = torch.exp(-r)
    if kind == "matern12":
        return ex
    if kind == "matern32":
        return (1 + r) * ex
    if kind == "matern52":
        return (1 + r + s / 3) * ex
    raise ValueError(kind)


def dcov_ds(kind, s, param=0.0):
    """dk/ds.  Matern nu = 1/2 and PP q = 0 have a cusp at s = 0: the kernels define the value there as 0, and so does this."""
    if kind == "rbf":
        return -LN2 * torch.exp2(-s)
    if kind == "rq":
        return -param * (1 + s).pow(-param - 1)
    r = _safe_sqrt(s)
    rs = torch.where(r > 0, r, torch.ones_like(r))
    if kind == "pp":
        e, _, _, _, b0, b1, b2, sing = pp_shape(param)
        u = (1 - r).clamp_min(0)
        w = torch.where(u > 0, u.pow(e - 1), torch.zeros_like(u))
        return 0.5 * w * (b0 + b1 * r + b2 * r * r + torch.where(r > 0, sing / rs, torch.zeros_like(r)))
    ex = torch.exp(-r)
    if kind == "matern12":
        return torch.where(r > 0, -0.5 * ex / rs, torch.zeros_like(r))
    if kind == "matern32":
        return -0.5 * ex
    if kind == "matern52":
        return -(1 + r) * ex / 6
    raise ValueError(kind)


def dcov_dalpha(s, alpha):
    """RQ: dk/dalpha at fixed s = -(1 + s)^-alpha ln(1 + s)."""
    return -(1 + s).pow(-alpha) * torch.log1p(s)


def sqdiff(a, b):
    """(a_i - b_j)^2 per column: [..., n, m, dp] of prepared rows a [..., n, dp], b [..., m, dp]"""
    return (a.double().unsqueeze(-2) - b.double().unsqueeze(-3)).pow(2)


def sqdist(a, b):
    return sqdiff(a, b).sum(-1)


def cov(kind, a, b, param=0.0):
    """K [..., n, m] of PREPARED rows a [..., n, dp], b [..., m, dp]."""
    if kind == "prod":
        ka, kb, da = prod_shape(param)
        d2 = sqdiff(a, b)
        return cov_s(BASE[ka], d2[..., :da].sum(-1)) * cov_s(BASE[kb], d2[..., da:].sum(-1))
    if kind == "add":
        valid = ~torch.isnan(a.double())                         # [..., n, dp]: the padding columns of the left row are not counted
        d2 = sqdiff(torch.nan_to_num(a.double()), torch.nan_to_num(b.double()))
        terms = cov_s(BASE[int(param)], d2) * valid.unsqueeze(-2)
        return terms.sum(-1) / valid.sum(-1, keepdim=True)
    return cov_s(kind, sqdist(a, b), param)


def cov_diag(kind, a, b, param=0.0):
    """k(a_i, b_i): [n]"""
    return cov(kind, a.unsqueeze(-2), b.unsqueeze(-2), param).reshape(a.shape[:-1])


def grad_block(kind, a, b, param, W):
    """gpamd_kernel_grad_block: (W dk/ds, sum W k, sum W dk/dalpha) for the rows a [nrows, dp] against b [m, dp]; the last is 0 unless RQ."""
    s, W = sqdist(a, b), W.double()
    acc1 = (W * dcov_dalpha(s, param)).sum() if kind == "rq" else torch.zeros((), dtype=F64)
    return W * dcov_ds(kind, s, param), (W * cov_s(kind, s, param)).sum(), acc1


def grad_batched(kind, A, B, params, W):
    """gpamd_kernel_grad_batched: G [b, 2 + dp] = (sum W k | sum W dk/ds (z_iq - z_jq)^2, q < dp | sum W dk/dalpha), member g with params[g]."""
    nb, dp = A.shape[0], A.shape[-1]
    G = torch.zeros(nb, 2 + dp, dtype=F64)
    for g in range(nb):
        p = 0.0 if params is None else float(params[g])
        d2 = sqdiff(A[g], B[g])
        s, Wg = d2.sum(-1), W[g].double()
        G[g, 0] = (Wg * cov_s(kind, s, p)).sum()
        G[g, 1:1 + dp] = ((Wg * dcov_ds(kind, s, p)).unsqueeze(-1) * d2).sum((0, 1))
        if kind == "rq":
            G[g, 1 + dp] = (Wg * dcov_dalpha(s, p)).sum()
    return G
