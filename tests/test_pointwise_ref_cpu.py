"""CPU: tests/pointwise_ref.py (the oracle of test_gpu_pointwise.py) against the restatements the suite already trusts, on RAW inputs at 1e-12 --
oracle/kernels.py (rbf, matern, rq), tests/piecewise_ref.py, tests/product_ref.py, tests/additive_ref.py -- and its derivatives and derivative
reductions against float64 autograd of its own ``cov``."""
import math

import pytest
import torch

from oracle import kernels as OK
from tests import additive_ref as AR
from tests import piecewise_ref as PR
from tests import pointwise_ref as R
from tests import product_ref as QR

F64 = torch.float64
TOL = 1e-12


def clouds(seed, n, m, d):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=F64), torch.randn(m, d, generator=g, dtype=F64), 0.5 + torch.rand(d, generator=g, dtype=F64)


def close(got, ref, what):
    err = float((got - ref).abs().max())
    assert err <= TOL, f"{what}: {err:.3e}"


@pytest.mark.parametrize("d,ard", [(1, False), (3, True), (7, False), (35, True)])
def test_single_parameter_families_vs_oracle(d, ard):
    x1, x2, ls = clouds(d, 23, 31, d)
    ls = ls if ard else ls[:1]
    dp = (d + 3) // 4 * 4
    shift = x1.mean(0)
    for kind, ref in (("rbf", OK.rbf(x1, x2, ls, direct=True)), ("matern12", OK.matern(x1, x2, ls, 0.5, direct=True)),
                      ("matern32", OK.matern(x1, x2, ls, 1.5, direct=True)), ("matern52", OK.matern(x1, x2, ls, 2.5, direct=True)),
                      ("rq", OK.rq(x1, x2, ls, 1.7, direct=True))):
        p = 1.7 if kind == "rq" else 0.0
        for sh in (None, shift):
            a, b = R.prep(kind, x1, ls, sh, p, dp), R.prep(kind, x2, ls, sh, p, dp + 4)[:, :dp]
            assert bool((a[:, d:] == 0).all())
            close(R.cov(kind, a, b, p), ref, f"{kind} d={d}")
            close(R.cov_diag(kind, a[:20], b[:20], p), ref.diagonal()[:20], f"{kind} diag")


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_piecewise_vs_ref(q):
    for d in (1, 3, 6):
        x1, x2, ls = clouds(10 * q + d, 23, 31, d)
        ls = 2.0 * math.sqrt(d) * ls   # (support radius = one lengthscale: keep a good share of the pairs inside it)
        code = 4 * PR.pp_j(d, q) + q
        dp = (d + 3) // 4 * 4
        ref = PR.pp_cov(x1, x2, ls, q)
        assert 0.1 < float((ref > 0).double().mean()) < 1.0
        close(R.cov("pp", R.prep("pp", x1, ls, None, code, dp), R.prep("pp", x2, ls, None, code, dp), code), ref, f"pp q={q} d={d}")


def test_pp_q2_coefficient_is_the_executed_one():
    assert R.pp_shape(4 * 3 + 2)[2] == (3 + 4 * 3 + 3) / 3 and R.pp_shape(4 * 3 + 2)[2] != (3 * 3 + 4 * 3 + 3) / 3


@pytest.mark.parametrize("ka,kb", QR.PAIRS)
def test_product_vs_ref(ka, kb):
    for da, db in ((1, 1), (1, 3), (2, 3), (3, 3)):
        d = da + db
        x1, x2, ls = clouds(ka + 4 * kb + 16 * da, 23, 31, d)
        code = ka + 4 * kb + 16 * da
        dp = (d + 3) // 4 * 4
        a, b = R.prep("prod", x1, ls, None, code, dp), R.prep("prod", x2, ls, None, code, dp)
        assert bool((a[:, d:] == 0).all())
        close(R.cov("prod", a, b, code), QR.prod_cov(ka, kb, da, x1, x2, ls), f"prod {code}")


@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_additive_vs_ref(base):
    for d in (2, 3, 4, 5, 8):
        x1, x2, ls = clouds(base + 4 * d, 23, 31, d)
        dp = (d + 3) // 4 * 4
        a, b = R.prep("add", x1, ls, None, base, dp), R.prep("add", x2, ls, None, base, dp)
        assert bool(torch.isnan(a[:, d:]).all()) and a[:, d:].numel() == 23 * (dp - d) and not bool(torch.isnan(a[:, :d]).any())
        close(R.cov("add", a, b, base), AR.add_mean(base, x1, x2, ls), f"add base={base} d={d}")
        close(R.cov_diag("add", a, a, base), torch.ones(23, dtype=F64), "add diagonal")


def test_prep_isotropic_is_ard_with_equal_lengthscales_and_ldx_free():
    x1, _, ls = clouds(0, 9, 9, 5)
    for kind, p in (("rbf", 0.0), ("rq", 2.5), ("pp", 13)):
        one = R.prep(kind, x1, ls[:1], None, p, 8)
        assert torch.equal(one, R.prep(kind, x1, ls[:1].expand(5), None, p, 8))
    assert abs(R.coef("rbf") - math.sqrt(0.5 * math.log2(math.e))) < 1e-16 and abs(R.coef("rq", 3.0) - 1 / math.sqrt(6.0)) < 1e-16
    assert abs(R.coef("rbf", 0.0, torch.float32) - R.coef("rbf")) < 1e-7 and R.coef("rbf", 0.0, torch.float32) != R.coef("rbf")


PARAMS = [("rbf", 0.0), ("matern12", 0.0), ("matern32", 0.0), ("matern52", 0.0), ("rq", 1.7), ("pp", 4 * 1 + 0), ("pp", 4 * 2 + 0), ("pp", 4 * 2 + 1),
          ("pp", 4 * 3 + 2), ("pp", 4 * 4 + 3)]


@pytest.mark.parametrize("kind,p", PARAMS)
def test_derivatives_vs_autograd(kind, p):
    g = torch.Generator().manual_seed(5)
    s = (torch.rand(4000, generator=g, dtype=F64) * (1.5 if kind == "pp" else 9.0) + 1e-3).requires_grad_(True)
    k = R.cov_s(kind, s, p)
    (dk,) = torch.autograd.grad(k.sum(), s)
    got = R.dcov_ds(kind, s.detach(), p)
    assert float(((got - dk).abs() / (1 + dk.abs())).max()) <= TOL
    if kind == "pp":
        assert bool((got[s.detach() >= 1] == 0).all()) and bool((got[s.detach() < 0.99] != 0).all())
    if kind == "rq":
        al = torch.tensor(p, dtype=F64, requires_grad=True)
        (da,) = torch.autograd.grad(R.cov_s("rq", s.detach(), al).sum(), al)
        assert abs(float(R.dcov_dalpha(s.detach(), p).sum() - da)) <= TOL * float(R.dcov_dalpha(s.detach(), p).abs().sum())


def test_cusps_are_zero_at_coincident_points():
    z = torch.zeros(3, dtype=F64)
    for kind, p in (("matern12", 0.0), ("pp", 4), ("pp", 8)):
        assert bool((R.dcov_ds(kind, z, p) == 0).all()) and bool((R.cov_s(kind, z, p) == 1).all())
    for kind, p in (("rbf", 0.0), ("matern32", 0.0), ("matern52", 0.0), ("rq", 2.0), ("pp", 9), ("pp", 14), ("pp", 19)):
        assert bool(torch.isfinite(R.dcov_ds(kind, z, p)).all()) and bool((R.dcov_ds(kind, z, p) < 0).all())


@pytest.mark.parametrize("kind,p", PARAMS[:6] + PARAMS[7:8])
def test_reductions_vs_autograd(kind, p):
    """grad_block: acc[0] is sum W k and W dk/ds its derivative by s; grad_batched: G[1 + q] is half the derivative of sum W k by a scale of column q."""
    g = torch.Generator().manual_seed(11)
    nb, n, m, dp = 2, 5, 7, 4
    A, B = 0.4 * torch.randn(nb, n, dp, generator=g, dtype=F64), 0.4 * torch.randn(nb, m, dp, generator=g, dtype=F64)
    W = torch.randn(nb, n, m, generator=g, dtype=F64)
    ps = [p, p * 1.5 if kind == "rq" else p]
    G = R.grad_batched(kind, A, B, ps if kind in ("rq", "pp") else None, W)
    for b in range(nb):
        c = torch.ones(dp, dtype=F64, requires_grad=True)
        al = torch.tensor(float(ps[b]), dtype=F64, requires_grad=True)
        val = (W[b] * R.cov(kind, A[b] * c, B[b] * c, al if kind == "rq" else ps[b])).sum()
        grads = torch.autograd.grad(val, [c, al], allow_unused=True)
        sabs = float((W[b].abs() * R.cov(kind, A[b], B[b], ps[b])).sum())
        assert abs(float(G[b, 0] - val.detach())) <= TOL * sabs
        assert float((G[b, 1:1 + dp] - 0.5 * grads[0]).abs().max()) <= 1e-11 * sabs
        assert abs(float(G[b, 1 + dp]) - (float(grads[1]) if kind == "rq" else 0.0)) <= 1e-11 * sabs
        Wd, a0, a1 = R.grad_block(kind, A[b, 1:4], B[b], ps[b], W[b, 1:4])
        assert abs(float(a0 - (W[b, 1:4] * R.cov(kind, A[b, 1:4], B[b], ps[b])).sum())) <= TOL * sabs
        assert torch.equal(Wd, W[b, 1:4] * R.dcov_ds(kind, R.sqdist(A[b, 1:4], B[b]), ps[b]))
        # sum_q of the per-column sums is sum W dk/ds s
        assert abs(float(G[b, 1:1 + dp].sum() - (W[b] * R.dcov_ds(kind, R.sqdist(A[b], B[b]), ps[b]) * R.sqdist(A[b], B[b])).sum())) <= 1e-11 * sabs
        assert (kind == "rq") == (float(a1) != 0.0)
