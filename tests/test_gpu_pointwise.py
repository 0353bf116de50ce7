"""The point-wise, generic row-block and stacked-batch kernels, ONE ENTRY POINT PER CASE, through the C ABI (``gpytorch_amd._lib.lib()``) only.
Reference: tests/pointwise_ref.py (float64, tied to the older restatements and to autograd in tests/test_pointwise_ref_cpu.py), evaluated ON THE
PREPARED ROWS THE KERNEL READ (the float32 rows upcast), so a tolerance is the kernel's own arithmetic and nothing else.

Entry points exercised:
  gpamd_prep_points_f32 gpamd_prep_points_f64 gpamd_kernel_rows_f32 gpamd_kernel_dense_f32 gpamd_kernel_diag_f32 gpamd_kernel_rows_f64
  gpamd_kernel_diag_f64 gpamd_kernel_grad_block_f32 gpamd_kernel_grad_block_f64 gpamd_kernel_dense_batched_f32 gpamd_kernel_grad_batched_f32
  gpamd_pivoted_cholesky_f32

Every case (the conventions of tests/test_gpu_solver_steps.py): inputs from a seeded generator; every leading dimension once tight and once + 8,
NaN in every input pad and a sentinel in every pure output pad; everything an entry point must not write BITWISE unchanged; every case run twice
from the same state, bitwise equal wherever no floating-point atomic is involved.

TOLERANCES -- derived from the kernels' stated arithmetic, never measured.  u = 2^-24 (unit roundoff of float32; eps32 = 2 u).
  * prep_points: (x - shift) * (coef / l) is three roundings: |got - ref| <= gamma_3 |ref|, gamma_3 = 3 u / (1 - 3 u), the reference taking `coef` as the
    host holds it (one float32 sqrt / quotient: pointwise_ref.coef(..., float32)).  float64: 4 eps64 |ref|.  Padding: exactly 0 / NaN.
  * float32 covariance entries: a running first-order error analysis of the kernel's own operation sequence (csrc/common.hpp cov_from_sq, dcov_dsq,
    pp_cov, pp_dcov; csrc/misc_kernels.hpp cov_pair).  ``f32_model`` restates that sequence in float64 with one named rounding step per operation;
    the bound of an entry is the sum over the steps of |value with that step's result off by its maximal relative error - value|, times 1.05 for the
    second-order terms, + 1e-36 (denormals are flushed).  The steps and their maximal errors:
      - s = |z - z'|^2: the differences are rounded (2 u on each square), then dp fused multiply-adds: (dp + 2) u relative -- all terms are
        non-negative, so the bound is relative to s; the kernels that square and add separately (grad_batched; grad_block unless contracted): (dp + 3) u;
      - v_sqrt_f32, v_exp_f32, v_log_f32: 1 ulp = 2 u; a float32 quotient: 2.5 ulp = 5 u; every other operation u; a product with a rounded constant 1.5 u;
      - PP: the Horner polynomial's three fused multiply-adds on coefficients that are themselves a few float32 operations: 6 u of sum |terms|.
    Propagated through k by the model: the sensitivity |s k'(s)| is bounded for every family (1/e for RBF / RQ / Matern-1/2, <= 0.95 for the others); RQ adds
    alpha u (the rounding of 1 + s under the power); PP carries e = j + q (the rounding of 1 - r under the power).  The product family: both factors'
    bounds, each weighted with the other factor, + u; the additive family: the mean of the per-column bounds (dp = 1 each) + (d + 5) u for the sum and the
    quotient.  Then out = scale * k (+ dadd): one more u |out| each.  The test asserts that no derived bound exceeds 4e-6 scale, the value
    tests/test_gpu_kv.py holds these kernels to.
  * float64 entries: 1e-12 scale; W dk/ds: 1e-12 |w| (1 + |dk/ds|).
  * reductions (acc, G: sums in double of float32 terms; grad_batched first adds up to GB_ROWS = 32 rows per thread in float32):
      delta_k sum|w| + (GB_ROWS + 2) u sum|terms| + 1e-12 sum|terms|,   delta_k = the largest entry bound of the block
    (grad_block: no middle term, its products are formed in double); the per-column sums of grad_batched: the entry is dk/ds (z_iq - z_jq)^2, whose
    square adds 3 u and the product w dk/ds one more.  float64: 1e-12 sum|terms|.
  * pivoted Cholesky: the method of test_pivoted_cholesky_vs_oracle (tests/test_gpu_bbmm.py): the device's pivots replayed in the float64 oracle, every
    one an arg-max within 1e-5 scale, the factor within 1e-3; on the exact-arithmetic clouds pivots, stopping step and factor must match EXACTLY.

OBSERVED on an MI355X (for orientation only; nothing asserts against it): the largest |got - ref| over all cases of a family in units of eps32 scale,
the derived bound at that entry in brackets.  ``within`` prints the largest error of every float32 comparison and its bound (run with -s and take the maxima).
  k:      rbf 1.56 (7.1)   matern12 0.96 (4.4)   matern32 1.76 (3.9)   matern52 2.18 (5.2)   rq 4.23 (5.7; alpha = 8 in the stacked batch)
          pp q=0 1.41 (6.2)   q=1 2.02 (7.4)   q=2 2.56 (8.7)   q=3 3.20 (10.1)   prod 1.71 (5.8)   add 1.53 (10.0)
  dk/ds:  rbf 1.86 (4.6)   matern12 5.88 (66.5)   matern32 0.97 (7.2)   matern52 0.72 (2.4)   rq 6.18 (12.3)   pp q=0 16.5 (116)   q=1 18.1 (120)
          (the absolute error of W dk/ds with W ~ N(0, 1), in eps32; dk/ds itself is of order e^2 for PP and unbounded towards r = 0 for Matern-1/2 and PP q = 0)
No observed error exceeds its derived bound, and every derived bound of k is below the 4e-6 cap (asserted in ``scaled``).
"""
import ctypes as C
import math

import pytest
import torch

from oracle import pivoted_cholesky as OPC
from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN, SENT = float("nan"), -1234.5
EINVAL, EUNSUPPORTED = -1, -2
U = 2.0 ** -24
E32, E64 = torch.finfo(F32).eps, torch.finfo(F64).eps
CAP = 4e-6          # tests/test_gpu_kv.py: no derived float32 entry bound may exceed this (times scale)
GB_ROWS = 32        # csrc/extra_batch.hip
LN2, LOG2E = math.log(2.0), 1.4426950408889634
SIX = [("rbf", 0.0), ("matern12", 0.0), ("matern32", 0.0), ("matern52", 0.0), ("rq", 1.75), ("pp", 4 * 3 + 1)]
M_EDGES = [1, 255, 256, 257, 513]


def lib():
    from gpytorch_amd._lib import lib as _lib

    return _lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(x):
    x = x.contiguous()
    return x.view(torch.int32) if x.dtype == F32 else (x.view(torch.int64) if x.dtype == F64 else x)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def pad_is(buf, n, fill):
    return same(buf[..., n:], torch.full_like(buf[..., n:], fill))


def within(got, ref, bound, what, fam=None, unit=1.0):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    if fam is not None and err.numel():
        i = int(err.argmax())
        print(f"[observed] {fam} {float(err.flatten()[i]) / (E32 * unit):.2f} ({float(bound.flatten()[i]) / (E32 * unit):.1f})")   # in eps32 * unit; asserts nothing
    bad = err > bound
    if bool(bad.any()):
        i = int((err - bound).argmax())
        raise AssertionError(f"{what}: |got - ref| = {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} (ref {float(ref.flatten()[i]):.6e}, "
                             f"{int(bad.sum())} of {bad.numel()} elements)")


def twice(run, loose=()):
    """run the case twice from the same preset state: bitwise-equal results (but the keys in ``loose``: sums through floating-point atomics)"""
    a, b = run(), run()
    for k in a:
        assert k in loose or same(a[k], b[k]), f"{k}: not bitwise reproducible run to run"
    return a, b


# =========================================================================================== the float32 arithmetic model (module docstring)
class _Steps:
    """st(x, h): the result x of one rounded operation; the `target`-th such result is taken off by h u relative (st.add: by h u mag absolute)"""

    def __init__(self, target):
        self.i, self.target = 0, target

    def __call__(self, x, h):
        self.i += 1
        return x * (1.0 + h * U) if self.i - 1 == self.target else x

    def add(self, x, h, mag):
        self.i += 1
        return x + h * U * mag if self.i - 1 == self.target else x


def f32_model(kind, s, p, what, target, D):
    """(value, number of steps): k (``what`` = "k"), dk/ds ("g") or RQ's dk/dalpha ("a") as the float32 kernels evaluate it, in float64"""
    st = _Steps(target)
    s = st(s, D)
    zero = torch.zeros_like(s)
    if kind == "rbf":
        k = st(torch.exp2(-s), 2)
        out = k if what == "k" else st(-LN2 * k, 1.5)
    elif kind == "rq":
        L = st(torch.log2(st(1 + s, 1)), 2)
        if what == "g":
            out = st(-p * st(torch.exp2(st(-st(p + 1.0, 1) * L, 1)), 2), 1)
        else:
            out = st(torch.exp2(st(-p * L, 1)), 2)
            if what == "a":   # -k ln2 log2(1 + s)
                out = st(st(-out * LN2, 1.5) * L, 1)
    elif kind == "pp":
        e, c1, c2, c3, b0, b1, b2, sing = R.pp_shape(p)
        r = st(R._safe_sqrt(s), 2)
        u = st(1 - r, 1).clamp_min(0)
        L = st(torch.log2(u), 2)
        if what == "k":
            w = st(torch.exp2(st(L * e, 1)), 2)
            out = st(w * st(1 + r * (c1 + r * (c2 + r * c3)), 6), 1)
        else:
            w = torch.where(u > 0, st(torch.exp2(st(torch.where(u > 0, L, zero) * (e - 1), 1)), 2), zero)
            poly = st.add(b0 + r * (b1 + r * b2), 6, abs(b0) + r * (abs(b1) + r * abs(b2)))
            rs = torch.where(r > 1e-15, r, torch.ones_like(r))
            sg = torch.where(r > 1e-15, st(sing / rs, 5), zero) if sing else zero
            out = st(0.5 * w * st(poly + sg, 1), 1)
    else:
        r = st(R._safe_sqrt(s), 2)
        ex = st(torch.exp2(st(-r * LOG2E, 1.5)), 2)
        if kind == "matern12":
            rs = torch.where(r > 1e-15, r, torch.ones_like(r))
            out = ex if what == "k" else torch.where(r > 1e-15, st(-0.5 * ex / rs, 5), zero)
        elif kind == "matern32":
            out = st(st(1 + r, 1) * ex, 1) if what == "k" else -0.5 * ex
        else:
            r1 = st(1 + r, 1)
            out = st(st(s * (1.0 / 3.0) + r1, 1.5) * ex, 1) if what == "k" else st(st(-r1 * ex, 1) * (1.0 / 6.0), 1.5)
    return out, st.i


def entry_bound(kind, s, p, what, D):
    """|float32 kernel value - exact value| <= this, per entry (s: exact squared distances of the rows the kernel read, float64)"""
    base, nsteps = f32_model(kind, s, p, what, None, D)
    tot = torch.zeros_like(s)
    for t in range(nsteps):
        tot += (f32_model(kind, s, p, what, t, D)[0] - base).abs()
    return 1.05 * tot + 1e-36


def cov_bound(kind, a, b, p, D=None):
    """entry bound of k for prepared rows a [..., n, dp], b [..., m, dp] of any point-wise family (fused multiply-add distance: D = dp + 2)"""
    dp = a.shape[-1]
    D = dp + 2 if D is None else D
    if kind == "prod":
        ka, kb, da = R.prod_shape(p)
        d2 = R.sqdiff(a, b)
        sa, sb = d2[..., :da].sum(-1), d2[..., da:].sum(-1)
        return (R.cov_s(R.BASE[kb], sb) * entry_bound(R.BASE[ka], sa, 0.0, "k", D) + R.cov_s(R.BASE[ka], sa) * entry_bound(R.BASE[kb], sb, 0.0, "k", D)
                + U * R.cov("prod", a, b, p))
    if kind == "add":
        valid = ~torch.isnan(a.double())
        d2 = R.sqdiff(torch.nan_to_num(a.double()), torch.nan_to_num(b.double()))
        cnt = valid.sum(-1, keepdim=True)
        return (entry_bound(R.BASE[int(p)], d2, 0.0, "k", 3) * valid.unsqueeze(-2)).sum(-1) / cnt + (cnt + 5) * U * R.cov("add", a, b, p)
    return entry_bound(kind, R.sqdist(a, b), p, "k", D)


def scaled(ref, bound, sc, extra=1):
    """out = scale * k: `extra` more roundings"""
    assert float(bound.max()) <= CAP, f"the derived bound {float(bound.max()):.3e} exceeds the cap {CAP:.1e}"
    return sc * ref, abs(sc) * bound + extra * U * (sc * ref).abs()


# ============================================================================================================================ clouds
def cloud(seed, N, d, dp, kind="rbf", dtype=F32):
    """prepared rows [N, dp]: d valid columns with |z - z'| on both sides of 1 (PP: exact zeros beyond), zero padding (additive: NaN);
    row 2 coincides with row 0 and the last row with row 1 (off-diagonal pairs at distance 0)"""
    z = torch.full((N, dp), NAN if kind == "add" else 0.0, dtype=dtype)
    z[:, :d] = (torch.randn(N, d, generator=gen(seed), dtype=F64) * (0.6 / math.sqrt(d))).to(dtype)
    if N >= 3:
        z[2] = z[0]
    if N >= 5:
        z[N - 1] = z[1]
    return z


POINTWISE = ([(k, p, dp, dp - 1) for k, p in SIX[:5] for dp in (4, 16, 32)]
             + [("pp", 4 * (q + 1 + dp // 8) + q, dp, dp - 1) for q in (0, 1, 2, 3) for dp in ((4, 16, 32) if q == 1 else (4,))]
             + [("prod", 0 + 4 * 2 + 16 * 2, 8, 5), ("prod", 1 + 4 * 3 + 16 * 1, 4, 3)]
             + [("add", base, dp, d) for base, dp, d in ((0, 4, 3), (1, 8, 6), (2, 4, 2), (3, 8, 8))])


def fam(kind, p):
    return f"pp{int(p) & 3}" if kind == "pp" else (f"add{int(p)}" if kind == "add" else (f"prod{int(p)}" if kind == "prod" else kind))


# ============================================================================================================== rows / dense / diag, f32
@pytest.mark.parametrize("kind,p,dp,d", POINTWISE, ids=[f"{fam(k, p)}-dp{dp}" for k, p, dp, _ in POINTWISE])
def test_rows_dense_diag_f32(dev, kind, p, dp, d):
    L, kid = lib(), R.KIND_ID[kind]
    N = 513
    Z = cloud(dp + int(p), N, d, dp, kind)
    Y = cloud(dp + int(p) + 1, N, d, dp, kind)
    Zd, Yd = Z.to(dev), Y.to(dev)
    Kz, Bz = R.cov(kind, Z[:70], Z, p), cov_bound(kind, Z[:70], Z, p)      # X1p = the first rows of X2p's cloud: out[i][i] is a diagonal entry
    Ky, By = R.cov(kind, Z[:70], Y, p), cov_bound(kind, Z[:70], Y, p)      # X2p = another cloud: K is not symmetric, the roles of the two clouds show
    assert not torch.allclose(Ky[:70, :70], Ky[:70, :70].t())
    if kind == "pp":
        assert bool((Kz == 0).any()) and float((Kz > 0).double().mean()) > 0.2, "the cloud must straddle r = 1"
    scd = torch.tensor([1.75], device=dev)
    for m in M_EDGES:
        for n in (1, 3, 70):
            for pad in (0, 8):
                for sc, other in ((None, False), (1.75, False), (1.75, True)):
                    ldo = m + pad
                    X2d, Kx, Bx = (Yd, Ky, By) if other else (Zd, Kz, Bz)
                    ref, bound = scaled(Kx[:n, :m], Bx[:n, :m], 1.0 if sc is None else 1.75, 0 if sc is None else 1)

                    def run_dense():
                        out = torch.full((n + 1, ldo), SENT, device=dev)
                        assert L.gpamd_kernel_dense_f32(kid, p, P(Zd), n, P(X2d), m, dp, P(scd) if sc else None, P(out), ldo, stream()) == 0
                        return dict(out=out.cpu())

                    out = twice(run_dense)[0]["out"]
                    within(out[:n, :m], ref, bound, f"dense m={m} n={n} other={other}", fam(kind, p), sc or 1.0)
                    assert pad_is(out[:n], m, SENT) and pad_is(out[n:], 0, SENT)
                    for i in range(0 if other else min(n, m)):
                        assert float(out[i, i]) == (sc or 1.0), "k(x, x) must be exactly scale"
                    if m >= 3 and n >= 3 and not other:
                        assert float(out[2, 0]) == (sc or 1.0) and float(out[0, 2]) == (sc or 1.0), "coincident off-diagonal pair"
                    # rows: unsorted, one index repeated
                    idx = torch.tensor([[5], [2, 0, 2]][n // 3] if n < 70 else torch.randperm(70, generator=gen(m)).tolist()[:69] + [11])
                    idxd = idx.to(dev)

                    def run_rows():
                        out = torch.full((n + 1, ldo), SENT, device=dev)
                        assert L.gpamd_kernel_rows_f32(kid, p, P(Zd), P(idxd), n, P(X2d), m, dp, P(scd) if sc else None, P(out), ldo, stream()) == 0
                        return dict(out=out.cpu())

                    out = twice(run_rows)[0]["out"]
                    refr, boundr = scaled(Kx[idx, :m], Bx[idx, :m], 1.0 if sc is None else 1.75, 0 if sc is None else 1)
                    within(out[:n, :m], refr, boundr, f"rows m={m} n={n} other={other}", fam(kind, p), sc or 1.0)
                    assert pad_is(out[:n], m, SENT) and pad_is(out[n:], 0, SENT)
                    for r_, i in enumerate(idx.tolist()):
                        if i < m and not other:
                            assert float(out[r_, i]) == (sc or 1.0)
    # diag: the m edges as lengths, against another cloud and against itself
    Kd, Bd = R.cov_diag(kind, Z, Y, p), cov_bound(kind, Z.unsqueeze(1), Y.unsqueeze(1), p).reshape(-1)
    for m in M_EDGES:
        for sc in (None, 1.75):
            for other in (True, False):
                def run_diag():
                    out = torch.full((m + 4,), SENT, device=dev)
                    assert L.gpamd_kernel_diag_f32(kid, p, P(Zd), P(Yd) if other else P(Zd), m, dp, P(scd) if sc else None, P(out), stream()) == 0
                    return dict(out=out.cpu())

                out = twice(run_diag)[0]["out"]
                assert pad_is(out, m, SENT)
                if other:
                    ref, bound = scaled(Kd[:m], Bd[:m], 1.0 if sc is None else 1.75, 0 if sc is None else 1)
                    within(out[:m], ref, bound, f"diag m={m}", fam(kind, p), sc or 1.0)
                else:
                    assert bool((out[:m] == (sc or 1.0)).all()), "k(x, x) must be exactly scale"


def test_kernel_rows_refuses_and_backend_splits_long_index_lists(dev):
    """gpamd_kernel_rows_f32 refuses more than 65535 rows (the grid's y extent) before any launch; backend.kernel_rows goes in blocks of 65535, float32 and float64"""
    from gpytorch_amd import backend as B

    Z = cloud(7, 40, 3, 4)
    Zd = Z.to(dev)
    xp = B.PreparedPoints(Zd, 40, 3, 4, "matern32")
    idx = torch.randint(0, 40, (65535 + 300,), generator=gen(1))
    out = torch.full((8,), SENT, device=dev)
    assert lib().gpamd_kernel_rows_f32(2, 0.0, P(Zd), P(idx.to(dev)), idx.numel(), P(Zd), 3, 4, None, P(out), 3, stream()) == EUNSUPPORTED
    assert lib().gpamd_kernel_rows_f32(2, 0.0, P(Zd), P(idx.to(dev)), 2, P(Zd), 3, 4, None, P(out), 2, stream()) == EINVAL
    assert pad_is(out.cpu(), 0, SENT)
    sc = torch.tensor([1.75], device=dev)
    got = B.kernel_rows(xp, idx, xp, sc).cpu()
    assert got.shape == (idx.numel(), 40)
    K = R.cov("matern32", Z, Z)
    ref, bound = scaled(K[idx], cov_bound("matern32", Z, Z, 0.0)[idx], 1.75)
    within(got, ref, bound, "backend.kernel_rows over 65535 rows")
    assert B.kernel_rows(xp, idx[:0], xp, sc).shape == (0, 40)
    # float64 likewise
    xp64 = B.PreparedPoints(Zd.double(), 40, 3, 4, "matern32")
    got = B.kernel_rows(xp64, idx, xp64, sc).cpu()
    assert got.dtype == F64 and got.shape == (idx.numel(), 40)
    within(got, 1.75 * K[idx], 1e-12 * 1.75, "backend.kernel_rows over 65535 rows, float64")


# ================================================================================================================== prep_points f32 / f64
PREP = ([(k, p, dp, dp - 1) for k, p in SIX for dp in (4, 8, 16, 32)] + [("rbf", 0.0, 8, 8), ("prod", 1 + 4 * 3 + 16 * 2, 8, 5), ("prod", 0 + 4 * 2 + 16 * 1, 4, 4),
                                                                       ("add", 2, 8, 5), ("add", 0, 4, 2)])


@pytest.mark.parametrize("kind,p,dp,d", PREP, ids=[f"{fam(k, p)}-dp{dp}-d{d}" for k, p, dp, d in PREP])
def test_prep_points_f32(dev, kind, p, dp, d):
    L, kid = lib(), R.KIND_ID[kind]
    for n in sorted({1, 256 // dp - 1, 256 // dp, 256 // dp + 1, 2 * (256 // dp) + 3} - {0}):   # n dp on both sides of one 256-thread block (and of two)
        for padx in (0, 3):
            for nls in (1, d):
                for with_shift in (False, True):
                    g = gen(n + dp + nls)
                    x = torch.randn(n, d, generator=g)
                    ls = 0.5 + torch.rand(nls, generator=g)
                    sh = torch.randn(d, generator=g) if with_shift else None
                    xd = torch.full((n, d + padx), NAN)
                    xd[:, :d] = x
                    xd, lsd, shd = xd.to(dev), ls.to(dev), None if sh is None else sh.to(dev)

                    def run():
                        out = torch.full((n * dp + 4,), SENT, device=dev)
                        assert L.gpamd_prep_points_f32(kid, p, P(xd), n, d, d + padx, P(lsd), nls, P(shd), P(out), dp, stream()) == 0
                        return dict(out=out.cpu())

                    out = twice(run)[0]["out"]
                    assert pad_is(out, n * dp, SENT)
                    got = out[: n * dp].view(n, dp)
                    ref = R.prep(kind, x, ls, sh, p, dp, coef_dtype=F32)
                    within(got[:, :d], ref[:, :d], 3 * U / (1 - 3 * U) * ref[:, :d].abs(), f"prep n={n} ldx={d + padx} nls={nls} shift={with_shift}")
                    if kind == "add":
                        assert bool(torch.isnan(got[:, d:]).all()), "additive padding must be NaN, every column"
                    else:
                        assert same(got[:, d:], torch.zeros(n, dp - d)), "padding columns must be exactly +0"
                    if nls == 1 and kind != "prod":
                        # one lengthscale is d equal ones
                        ls_d = ls.expand(d).contiguous().to(dev)
                        out2 = torch.full((n * dp + 4,), SENT, device=dev)
                        assert L.gpamd_prep_points_f32(kid, p, P(xd), n, d, d + padx, P(ls_d), d, P(shd), P(out2), dp, stream()) == 0
                        assert same(out2.cpu()[: n * dp], out[: n * dp])
    if kind == "prod":   # the second coefficient from the split column on: the two column groups differ by exactly the two families' constants
        ka, kb, da = R.prod_shape(p)
        ones = torch.ones(1, d, device=dev)
        one = torch.ones(1, device=dev)
        out = torch.full((dp,), SENT, device=dev)
        assert L.gpamd_prep_points_f32(kid, p, P(ones), 1, d, d, P(one), 1, None, P(out), dp, stream()) == 0
        want = [R.coef(R.BASE[ka], 0.0, F32)] * da + [R.coef(R.BASE[kb], 0.0, F32)] * (d - da) + [0.0] * (dp - d)
        assert out.cpu().tolist() == torch.tensor(want, dtype=F32).tolist()


@pytest.mark.parametrize("kind,p", SIX, ids=[k for k, _ in SIX])
def test_prep_points_f64(dev, kind, p):
    L, kid = lib(), R.KIND_ID[kind]
    for dp, d in ((4, 3), (8, 8), (16, 13), (32, 29), (36, 35), (35, 35)):   # (no multiple-of-4 rule on the generic path: dp = 35 is accepted as it is)
        for n in sorted({1, 256 // dp, 256 // dp + 1, 2 * (256 // dp) + 3}):
            for padx in (0, 3):
                for nls in (1, d):
                    for with_shift in (False, True):
                        g = gen(n + dp + nls)
                        x = torch.randn(n, d, generator=g, dtype=F64)
                        ls = 0.5 + torch.rand(nls, generator=g, dtype=F64)
                        sh = torch.randn(d, generator=g, dtype=F64) if with_shift else None
                        xd = torch.full((n, d + padx), NAN, dtype=F64)
                        xd[:, :d] = x
                        xd, lsd, shd = xd.to(dev), ls.to(dev), None if sh is None else sh.to(dev)

                        def run():
                            out = torch.full((n * dp + 4,), SENT, device=dev, dtype=F64)
                            assert L.gpamd_prep_points_f64(kid, p, P(xd), n, d, d + padx, P(lsd), nls, P(shd), P(out), dp, stream()) == 0
                            return dict(out=out.cpu())

                        out = twice(run)[0]["out"]
                        assert pad_is(out, n * dp, SENT)
                        got = out[: n * dp].view(n, dp)
                        ref = R.prep(kind, x, ls, sh, p, dp)
                        within(got[:, :d], ref[:, :d], 4 * E64 * ref[:, :d].abs(), f"prep64 dp={dp} n={n} ldx={d + padx} nls={nls}")
                        assert same(got[:, d:], torch.zeros(n, dp - d, dtype=F64))
    # the product and the additive family are float32 only
    buf = torch.zeros(64, device=dev, dtype=F64)
    assert L.gpamd_prep_points_f64(6, 29.0, P(buf), 1, 3, 3, P(buf), 1, None, P(buf), 4, stream()) == EINVAL
    assert L.gpamd_prep_points_f64(8, 1.0, P(buf), 1, 3, 3, P(buf), 1, None, P(buf), 4, stream()) == EINVAL


# ===================================================================================================================== rows / diag, f64
@pytest.mark.parametrize("kind,p", SIX, ids=[k for k, _ in SIX])
@pytest.mark.parametrize("dp", [4, 36])
def test_rows_diag_f64(dev, kind, p, dp):
    L, kid = lib(), R.KIND_ID[kind]
    N = 513
    Z = cloud(dp, N, dp - 1, dp, kind, F64)
    Y = cloud(dp + 1, N, dp - 1, dp, kind, F64)
    Zd, Yd = Z.to(dev), Y.to(dev)
    K = R.cov(kind, Z[:80], Z, p)
    scd = torch.tensor([1.75], device=dev, dtype=F64)
    for m in M_EDGES:
        for n in (1, 3, 70):
            idx = torch.tensor([[5], [2, 0, 2]][n // 3] if n < 70 else torch.randperm(70, generator=gen(m)).tolist()[:69] + [11])
            idxd = idx.to(dev)
            for pad in (0, 8):
                for sc in (None, 1.75):
                    for row0 in (None, 0, 7):   # None: the `rows` pointer form
                        ldo = m + pad

                        def run():
                            out = torch.full((n + 1, ldo), SENT, device=dev, dtype=F64)
                            assert L.gpamd_kernel_rows_f64(kid, p, P(Zd), P(idxd) if row0 is None else None, row0 or 0, n, P(Zd), m, dp, P(scd) if sc else None,
                                                           P(out), ldo, stream()) == 0
                            return dict(out=out.cpu())

                        out = twice(run)[0]["out"]
                        ref = (sc or 1.0) * (K[idx, :m] if row0 is None else K[row0:row0 + n, :m])
                        within(out[:n, :m], ref, 1e-12 * (sc or 1.0), f"rows64 m={m} n={n} row0={row0}")
                        assert pad_is(out[:n], m, SENT) and pad_is(out[n:], 0, SENT)
                        if row0 is not None and row0 < m:
                            assert float(out[0, row0]) == (sc or 1.0), "k(x, x) must be exactly scale"
    Kd = R.cov_diag(kind, Z, Y, p)
    for m in M_EDGES:
        for sc in (None, 1.75):
            for other in (True, False):
                def run_diag():
                    out = torch.full((m + 4,), SENT, device=dev, dtype=F64)
                    assert L.gpamd_kernel_diag_f64(kid, p, P(Zd), P(Yd) if other else P(Zd), m, dp, P(scd) if sc else None, P(out), stream()) == 0
                    return dict(out=out.cpu())

                out = twice(run_diag)[0]["out"]
                assert pad_is(out, m, SENT)
                if other:
                    within(out[:m], (sc or 1.0) * Kd[:m], 1e-12 * (sc or 1.0), f"diag64 m={m}")
                else:
                    assert bool((out[:m] == (sc or 1.0)).all())


# ============================================================================================================= kernel_grad_block f32 / f64
# the six families + PP q = 0 (a cusp like Matern-1/2) with e - 1 = 0 and with e - 1 = 1
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,p", SIX + [("pp", 4 * 1 + 0), ("pp", 4 * 2 + 0)], ids=[fam(k, p) + (f"-j{int(p) >> 2}" if k == "pp" else "") for k, p in SIX + [("pp", 4), ("pp", 8)]])
def test_kernel_grad_block(dev, dtype, kind, p):
    L, kid = lib(), R.KIND_ID[kind]
    fn = L.gpamd_kernel_grad_block_f32 if dtype == F32 else L.gpamd_kernel_grad_block_f64
    for dp in (4, 36):
        X1, X2 = cloud(dp + 2, 12, dp - 1, dp, kind, dtype), cloud(dp + 3, 513, dp - 1, dp, kind, dtype)
        X1[0], X1[4], X1[7], X1[8], X1[11] = X2[0], X2[0], X2[0], X2[254], X2[256]   # coincident pairs in both row windows, either side of the j block edge
        X1d, X2d = X1.to(dev), X2.to(dev)
        S = R.sqdist(X1, X2)
        Kk, Kg = R.cov_s(kind, S, p), R.dcov_ds(kind, S, p)
        if dtype == F32:
            Bk, Bg = entry_bound(kind, S, p, "k", dp + 3), entry_bound(kind, S, p, "g", dp + 3)
            Ba = entry_bound(kind, S, p, "a", dp + 3) if kind == "rq" else None
            assert float(Bk.max()) <= CAP
        for m in M_EDGES:
            for nrows in (1, 5):
                for row0 in (0, 7):
                    for pad in (0, 8):
                        ldw = m + pad
                        W = torch.randn(nrows, m, generator=gen(m + nrows + row0), dtype=dtype)
                        Wp = torch.full((nrows + 1, ldw), NAN, dtype=dtype)
                        Wp[:nrows, :m] = W
                        acc0 = torch.tensor([3.25, -1.5], dtype=F64)
                        rows = slice(row0, row0 + nrows)

                        def run():
                            Wd, acc = Wp.to(dev), acc0.to(dev)
                            assert fn(kid, p, P(X1d), row0, nrows, P(X2d), m, dp, P(Wd), ldw, P(acc), stream()) == 0
                            return dict(W=Wd.cpu(), acc=acc.cpu())

                        one_block = nrows == 1 and m <= 256
                        a, b = twice(run, loose=() if one_block else ("acc",))
                        refW, ref0, ref1 = R.grad_block(kind, X1[rows], X2[:m], p, W)
                        k_, g_, wabs = Kk[rows, :m], Kg[rows, :m], W.double().abs()
                        t0 = (wabs * k_).sum()
                        if dtype == F32:
                            bw = wabs * Bg[rows, :m] + U * refW.abs()
                            b0 = float(Bk[rows, :m].max()) * wabs.sum() + 1e-12 * t0
                        else:
                            bw = 1e-12 * wabs * (1 + g_.abs())
                            b0 = 1e-12 * t0
                        for r_ in (a, b):
                            got = r_["W"]
                            assert bool(torch.isnan(got[:nrows, m:]).all()) and bool(torch.isnan(got[nrows:]).all()), "the pad of W was written"
                            within(got[:nrows, :m], refW, bw, f"grad_block W m={m} nrows={nrows} row0={row0}", fam(kind, p) + "-dk" if dtype == F32 else None)
                            # added onto the preset values, not written over them
                            within(r_["acc"][0], acc0[0] + ref0, b0 + 2 * E64 * abs(float(acc0[0])), f"grad_block acc[0] m={m} nrows={nrows} row0={row0}")
                            if kind == "rq":
                                t1 = (wabs * R.dcov_dalpha(S[rows, :m], p).abs()).sum()
                                b1 = (float(Ba[rows, :m].max()) * wabs.sum() if dtype == F32 else 0.0) + 1e-12 * t1
                                within(r_["acc"][1], acc0[1] + ref1, b1 + 2 * E64 * abs(float(acc0[1])), "grad_block acc[1]")
                            else:
                                assert same(r_["acc"][1:], acc0[1:]), "acc[1] must stay untouched for a family without a shape parameter"
                            if kind == "matern12" or (kind == "pp" and int(p) & 3 == 0):
                                coin = S[rows, :m] == 0
                                assert bool(coin.any()) and bool((got[:nrows, :m][coin] == 0).all()), "W dk/ds at coincident points must be exactly 0"


# ==================================================================================================== kernel_dense_batched / kernel_grad_batched
PP_CODES = [4 * 1 + 0, 4 * 3 + 1, 4 * 4 + 2, 4 * 5 + 3]
BATCH = [(k, dp) for k in ("rbf", "matern12", "matern32", "matern52", "rq", "pp") for dp in (4, 8, 16)]


def batch_case(kind, dp, n, m, b, seed):
    d = dp - 1
    X1 = torch.stack([cloud(seed + 10 * g, n, d, dp) for g in range(b)])
    X2 = torch.stack([cloud(seed + 10 * g + 5, m, d, dp) for g in range(b)])
    X1[:, 0] = X2[:, 0]            # a coincident pair on the diagonal ...
    X1[:, n - 1] = X2[:, 0]        # ... and one off it (n > 1)
    kp = {"rq": [1.75, 0.5, 8.0], "pp": [PP_CODES[(g + dp // 4) % 4] for g in range(3)]}.get(kind, [0.25, 0.5, 0.75])[:b]   # (ignored by the other families)
    return X1, X2, kp, [1.75, 0.625, 2.5][:b], [0.125, 0.03125, 0.25][:b]


@pytest.mark.parametrize("kind,dp", BATCH, ids=[f"{k}-dp{dp}" for k, dp in BATCH])
def test_kernel_dense_batched(dev, kind, dp):
    L, kid = lib(), R.KIND_ID[kind]
    combo = 0
    for n in (1, 31, 32, 33, 70):
        for m in (1, 255, 256, 257):
            for pad, b in ((0, 1), (0, 3), (8, 1), (8, 3)):
                combo += 1
                null = ("kparam", "scale", "dadd", None)[((combo - 1) // 4) % 4]   # each of the three NULL in turn, with every (pad, b)
                if null == "kparam" and kind in ("rq", "pp"):
                    null = None
                X1, X2, kp, sc, da = batch_case(kind, dp, n, m, b, combo)
                ldo = m + pad
                X1d, X2d = X1.to(dev), X2.to(dev)
                kpd, scd, dad = (None if null == nm else torch.tensor(v, dtype=F32, device=dev) for nm, v in (("kparam", kp), ("scale", sc), ("dadd", da)))

                def run():
                    out = torch.full((b * n + 1, ldo), SENT, device=dev)
                    assert L.gpamd_kernel_dense_batched_f32(kid, P(kpd), P(X1d), n, P(X2d), m, dp, b, P(scd), P(dad), P(out), ldo, stream()) == 0
                    return dict(out=out.cpu())

                out = twice(run)[0]["out"]
                assert pad_is(out[: b * n], m, SENT) and pad_is(out[b * n:], 0, SENT)
                for g in range(b):
                    p = kp[g] if kind in ("rq", "pp") else 0.0
                    s_ = 1.0 if null == "scale" else sc[g]
                    ref, bound = scaled(R.cov(kind, X1[g], X2[g], p), cov_bound(kind, X1[g], X2[g], p), s_, 0 if null == "scale" else 1)
                    if null != "dadd":   # on i == j only, in the rectangular case too
                        eye = torch.eye(n, m, dtype=F64)
                        ref = ref + da[g] * eye
                        bound = bound + U * ref.abs() * eye
                    within(out[g * n:(g + 1) * n, :m], ref, bound, f"dense_batched n={n} m={m} b={b} g={g} null={null}", fam(kind, p), s_)
                    if null == "dadd":
                        assert float(out[g * n, 0]) == s_, "k(x, x) must be exactly scale"


@pytest.mark.parametrize("kind,dp", BATCH, ids=[f"{k}-dp{dp}" for k, dp in BATCH])
def test_kernel_grad_batched(dev, kind, dp):
    L, kid = lib(), R.KIND_ID[kind]
    combo = 0
    for n in (1, 31, 32, 33, 70):
        for m in (1, 255, 256, 257):
            for pad, b in ((0, 1), (0, 3), (8, 1), (8, 3)):
                combo += 1
                X1, X2, kp, _, _ = batch_case(kind, dp, n, m, b, combo)
                null_kp = kind not in ("rq", "pp") and ((combo - 1) // 4) % 2 == 0
                ldw = m + pad
                W = torch.randn(b, n, m, generator=gen(combo))
                Wp = torch.full((b * n + 1, ldw), NAN)
                Wp[: b * n, :m] = W.reshape(b * n, m)
                X1d, X2d, Wd = X1.to(dev), X2.to(dev), Wp.to(dev)
                kpd = None if null_kp else torch.tensor(kp, dtype=F32, device=dev)

                def run():
                    G = torch.full((b * (2 + dp) + 2,), SENT, device=dev, dtype=F64)
                    assert L.gpamd_kernel_grad_batched_f32(kid, P(kpd), P(X1d), n, P(X2d), m, dp, b, P(Wd), ldw, P(G), stream()) == 0
                    return dict(G=G.cpu())

                one_wg = m <= 256 and n <= GB_ROWS   # one workgroup contributes per member: no atomic meets another
                a, b2 = twice(run, loose=() if one_wg else ("G",))
                assert same(Wd.cpu(), Wp), "W is an input"
                ps = kp if kind in ("rq", "pp") else None
                ref = R.grad_batched(kind, X1, X2, ps, W)
                for r_ in (a, b2):
                    assert pad_is(r_["G"], b * (2 + dp), SENT)
                    G = r_["G"][: b * (2 + dp)].view(b, 2 + dp)
                    for g in range(b):
                        p = kp[g] if kind in ("rq", "pp") else 0.0
                        d2 = R.sqdiff(X1[g], X2[g])
                        s_ = d2.sum(-1)
                        wabs = W[g].double().abs()
                        k_, g_ = R.cov_s(kind, s_, p), R.dcov_ds(kind, s_, p)
                        Bk, Bg = entry_bound(kind, s_, p, "k", dp + 3), entry_bound(kind, s_, p, "g", dp + 3)
                        assert float(Bk.max()) <= CAP, f"the derived bound {float(Bk.max()):.3e} exceeds the cap {CAP:.1e}"
                        red = (GB_ROWS + 2) * U + 1e-12
                        t0 = (wabs * k_).sum()
                        within(G[g, 0], ref[g, 0], float(Bk.max()) * wabs.sum() + red * t0, f"grad_batched G[{g}][0] n={n} m={m}")
                        ent = (Bg + 4 * U * g_.abs()).unsqueeze(-1) * d2                      # entry bound of dk/ds (z_iq - z_jq)^2, per column
                        tq = (wabs * g_.abs()).unsqueeze(-1) * d2
                        bq = ent.amax((0, 1)) * wabs.sum() + red * tq.sum((0, 1))
                        within(G[g, 1:1 + dp], ref[g, 1:1 + dp], bq + 1e-300, f"grad_batched G[{g}][1..dp] n={n} m={m}")
                        assert bool((G[g, dp] == 0).all()), "the padding column (zero in both clouds) contributes exactly 0"
                        if kind == "rq":
                            Ba = entry_bound(kind, s_, p, "a", dp + 3)
                            ta = (wabs * R.dcov_dalpha(s_, p).abs()).sum()
                            within(G[g, 1 + dp], ref[g, 1 + dp], float(Ba.max()) * wabs.sum() + red * ta, f"grad_batched G[{g}][1 + dp]")
                        else:
                            assert same(G[g, 1 + dp:], torch.zeros(1, dtype=F64)), "the shape-parameter slot must be exactly +0 for a family without one"


# ============================================================================================================================ pivoted Cholesky
def run_pc(dev, kind, p, Zp, scale, rank, tol, pad):
    """(L [rank_alloc][ldl] as left by the call, pivots, m): L prefilled with a sentinel"""
    L_ = lib()
    n, dp = Zp.shape
    ldl = n + pad
    Zd = Zp.to(dev)
    scd = None if scale is None else torch.tensor([scale], device=dev)
    rows = min(rank, 512) + 1

    def run():
        Lb = torch.full((rows, ldl), SENT, device=dev)
        piv = torch.full((rows,), -7, device=dev, dtype=torch.int64)
        fwork = torch.zeros(n + 4, device=dev)
        iwork = torch.zeros(2 + 2 * n, device=dev, dtype=torch.int32)
        assert L_.gpamd_pivoted_cholesky_f32(R.KIND_ID[kind], p, P(Zd), n, dp, P(scd), rank, tol, P(Lb), ldl, P(piv), P(fwork), P(iwork), stream()) == 0
        return dict(L=Lb.cpu(), piv=piv.cpu(), m=iwork[:1].cpu())

    a = twice(run)[0]
    m = int(a["m"][0])
    assert 1 <= m <= min(rank, n)
    assert pad_is(a["L"][:m], n, SENT) and pad_is(a["L"][m:], 0, SENT), "rows >= m and all pads must stay untouched"
    assert bool((a["piv"][m:] == -7).all())
    return a["L"][:m, :n], a["piv"][:m], m


def spread_cloud(seed, n, dp=4):
    """2-D prepared RBF coordinates, about 0.7 points per unit area: K is well conditioned, a full-rank factor exists in float32"""
    z = torch.zeros(n, dp)
    z[:, :2] = torch.rand(n, 2, generator=gen(seed)) * (1.2 * math.sqrt(n) + 1.0)
    return z


@pytest.mark.parametrize("n,rank", [(1, 1), (1, 3), (2, 5), (7, 7), (7, 9), (8, 8), (8, 20), (9, 4), (255, 40), (256, 256), (257, 40), (513, 40), (600, 512)])
def test_pivoted_cholesky_shapes(dev, n, rank):
    """values by the method of test_pivoted_cholesky_vs_oracle (tests/test_gpu_bbmm.py): only the shapes are new -- the two-kernel path (n < 8), n on both
    sides of 256 (one partial against two in the "last block decides" step), rank > n (clamped), rank == n, rank = 512"""
    Z = spread_cloud(n, n)
    Kd = 1.5 * R.cov("rbf", Z, Z)
    for pad in (0, 8):
        Lt, piv, m = run_pc(dev, "rbf", 0.0, Z, 1.5, rank, 1e-9, pad)
        assert m == min(rank, n) and len(set(piv.tolist())) == m and int(piv[0]) == 0
        Lref, _, gaps = OPC.pivoted_cholesky(torch.full((n,), 1.5, dtype=F64), lambda q: Kd[q], rank, 1e-9, forced_pivots=piv, return_gaps=True)
        assert Lref.shape[1] == m
        assert max(gaps) < 1e-5, gaps
        assert float((Lt.t().double() - Lref).abs().max()) < 1e-3 * float(Lref.abs().max())
        res = Kd - Lt.t().double() @ Lt.double()
        assert float(res.diagonal().min()) > -1e-4
        if m == n:
            assert float(res.abs().max()) < 1e-4, "a full-rank factor reproduces K"


@pytest.mark.parametrize("n", [5, 7, 8, 9, 300])
def test_pivoted_cholesky_identity(dev, n):
    """points so far apart that K = I in float32: pivots 0, 1, 2, ... and rows sqrt(scale) e_k, exactly"""
    Z = torch.zeros(n, 4)
    Z[:, 0] = 40.0 * torch.arange(n)      # s >= 1600: 2^-s is zero in float32
    for scale in (None, 4.0, 1.7):
        for pad in (0, 8):
            rank = min(n, 12)
            Lt, piv, m = run_pc(dev, "rbf", 0.0, Z, scale, rank, 1e-6, pad)
            assert m == rank and piv.tolist() == list(range(rank))
            want = torch.zeros(rank, n)
            want[torch.arange(rank), torch.arange(rank)] = torch.tensor(scale or 1.0).sqrt()
            assert same(Lt, want)


@pytest.mark.parametrize("n", [6, 8, 10, 258, 514])
def test_pivoted_cholesky_stops_at_an_exactly_known_step(dev, n):
    """pairs of identical points, far from every other pair: after one point of every pair the Schur complement is exactly zero, the factor stops at
    exactly m = n / 2 for any tol > 0; pivots and factor are those of the sequential oracle in the same (exact) arithmetic"""
    h = n // 2
    order = torch.randperm(n, generator=gen(n))
    Z = torch.zeros(n, 4)
    Z[order, 0] = 40.0 * (torch.arange(n) // 2)      # the twins sit at scattered indices
    K = R.cov("rbf", Z, Z)
    assert bool(((K == 0) | (K == 1)).all()) and int(K.sum()) == 2 * n
    for scale in (None, 4.0):      # (sqrt exact: the twin's residual is an exact zero)
        sc = scale or 1.0
        Lo, po = OPC.pivoted_cholesky(torch.full((n,), sc), lambda q: (sc * K[q]).float(), n, 1e-30, return_pivots=True)
        assert Lo.shape[1] == h
        for pad in (0, 8):
            for tol in (1e-30, 1e-3):
                Lt, piv, m = run_pc(dev, "rbf", 0.0, Z, scale, min(n, 512), tol, pad)
                assert m == h, f"stopped at {m}, the residual is exactly zero after {h}"
                assert piv.tolist() == po[:h].tolist()
                assert same(Lt, Lo.t().contiguous())


@pytest.mark.parametrize("tail", [[], [0.1, -0.1, 0.7]], ids=["two-kernel-n7", "fused-n10"])
def test_pivoted_cholesky_tie_rule(dev, tail):
    """ties resolve to the lowest POSITION in the current permutation, not to the lowest index: on this cloud (prepared 1-D RBF coordinates) the
    sequential oracle picks [0, 5, 2, 1]; the lowest index would give [0, 5, 1, 2]"""
    xs = [0.0, 1.0, -1.0, 0.5, -0.5, 100.0, 0.25] + tail
    n = len(xs)
    Z = torch.zeros(n, 4)
    Z[:, 0] = torch.tensor(xs)
    Kd = R.cov("rbf", Z, Z)
    _, po = OPC.pivoted_cholesky(torch.ones(n, dtype=F64), lambda q: Kd[q], n, 1e-9, return_pivots=True)
    assert po[:4].tolist() == [0, 5, 2, 1]
    for pad in (0, 8):
        Lt, piv, m = run_pc(dev, "rbf", 0.0, Z, None, 5, 1e-9, pad)   # (beyond a few steps the residuals of this cloud sink below float32 resolution)
        assert piv[:4].tolist() == [0, 5, 2, 1], piv.tolist()
        Lref, _, gaps = OPC.pivoted_cholesky(torch.ones(n, dtype=F64), lambda q: Kd[q], 5, 1e-9, forced_pivots=piv, return_gaps=True)
        assert Lref.shape[1] == m and max(gaps) < 1e-5, gaps
        assert float((Lt.t().double() - Lref).abs().max()) < 1e-3 * float(Lref.abs().max())
