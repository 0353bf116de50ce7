"""Fused float64 K*V for 17 .. 512 input dimensions (csrc/kv_f64_wide.hpp: Gram form on the float64 matrix pipe, run-time dimension loop) against a
float64 CPU reference: K by direct differences of the scaled inputs, then K @ V.

Tolerance per output entry, derived (kv_f64_wide.hpp, "Accuracy"), u = 2^-53, in prepared units:
    4 [ max|dk/ds| (dp + 4) u (max|z_i| + max|z_j|)^2 + (m + 64) u ] * outputscale * sum_j |V_jc|
the first term is the Gram form's error in s carried through the covariance, the second the m-term contraction; 4 covers the few-ulp exp / pow."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ALPHA = 1.7
SCALE = 1.3
DKDS = {"rbf": math.log(2.0), "rq": ALPHA, "matern32": 0.5, "matern52": 1.0 / 6.0}   # max |dk/ds|, prepared units (dcov_dsq_f64 at s = 0)
KINDS = list(DKDS)


def _cov(kind, x1, x2, ls):
    r = torch.cdist(x1 / ls, x2 / ls, compute_mode="donot_use_mm_for_euclid_dist")   # direct differences
    if kind == "rbf":
        return torch.exp(-0.5 * r * r)
    if kind == "rq":
        return (1.0 + r * r / (2.0 * ALPHA)) ** -ALPHA
    a = math.sqrt(3.0 if kind == "matern32" else 5.0) * r
    return ((1.0 + a) if kind == "matern32" else (1.0 + a + a * a / 3.0)) * torch.exp(-a)


def _case(kind, d, n, m, t, dev, ard=False, offset=0.0, shift=True, square=False):
    """(reference K @ V, V, prepared clouds, per-column bound); lengthscales ~ 0.4 sqrt(d), so that the typical entry of K is neither 0 nor 1"""
    from gpytorch_amd import backend as B

    g0 = torch.Generator().manual_seed(7 * d + n + m + t)
    ls = math.sqrt(d) * (0.35 + 0.1 * torch.rand(d if ard else 1, generator=g0, dtype=torch.float64))
    X1 = torch.rand(n, d, generator=g0, dtype=torch.float64) + offset * ls
    if square:
        X1[n // 2:] = X1[: n - n // 2]      # every point twice: s = 0 off the diagonal too
        X2 = X1
    else:
        X2 = torch.rand(m, d, generator=g0, dtype=torch.float64) + offset * ls
    V = torch.randn(m, t, generator=g0, dtype=torch.float64)
    K = SCALE * _cov(kind, X1, X2, ls)
    assert 0.05 <= float(K.median()) <= 0.9
    sh = X1.mean(0).to(dev) if shift else None
    param = ALPHA if kind == "rq" else None
    p1 = B.prep_points(kind, X1.to(dev), ls.to(dev), sh, param)
    p2 = p1 if square else B.prep_points(kind, X2.to(dev), ls.to(dev), sh, param)
    assert B.fused_f64(p1, p2) and p1.dp == B.padded_dim(d)
    zsum = float(p1.xp.norm(dim=1).max()) + float(p2.xp.norm(dim=1).max())
    bound = 4.0 * (DKDS[kind] * (p1.dp + 4) * U * zsum * zsum + (m + 64) * U) * SCALE * V.abs().sum(0)
    return K @ V, V, p1, p2, bound


def _product(p1, p2, V, dev):
    from gpytorch_amd import backend as B

    sc = torch.tensor([SCALE], dtype=torch.float64, device=dev)
    return B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev), torch.float64), scale=sc), p1.n).cpu()


def _check(out, ref, bound, factor=1.0):
    err = (out - ref).abs().amax(0)
    assert bool(torch.isfinite(out).all())
    assert bool((err <= factor * bound).all()), f"column {int((err / bound).argmax())}: {float((err / bound).max()):.3g} x the bound"


# d: 17 (stride 20, the first admitted), 28 (stride 32 > d), 33 (one column past two chunks), 100, 512;  n: past one / two 128-row blocks;  m: 200 (S = 1,
# ragged tail), 600 (S >= 2);  t: 1, 4 (VALU flavour), 5, 16, 17, 40 (CT = 1, 1, 2, 3), 65 (CT = 4 + a VALU column), 69 (two MFMA groups)
SHAPES = [(17, 130, 200, 1), (17, 257, 600, 65), (28, 130, 600, 4), (28, 257, 200, 69), (33, 257, 600, 5), (100, 130, 200, 16), (100, 257, 600, 40),
          (512, 130, 600, 17)]


@pytest.mark.parametrize("d,n,m,t", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_product(kind, d, n, m, t, dev):
    ref, V, p1, p2, bound = _case(kind, d, n, m, t, dev, ard=d in (28, 100))
    _check(_product(p1, p2, V, dev), ref, bound)


def test_extent(dev):
    """the cloud 30 lengthscales from the origin in every dimension, not centred: the |z|^2 term of the bound dominates, and the bound holds"""
    ref, V, p1, p2, bound = _case("rbf", 40, 130, 200, 5, dev, offset=30.0, shift=False)
    assert p1.zmax2 > 1e4
    _check(_product(p1, p2, V, dev), ref, bound)


@pytest.mark.parametrize("kind", ["matern32", "matern52"])
def test_coincident_points(kind, dev):
    """s = -O(u |z|^2) before the clamp, and the Matern branch takes a square root"""
    ref, V, p1, p2, bound = _case(kind, 40, 150, 150, 5, dev, square=True)
    _check(_product(p1, p2, V, dev), ref, bound)


def test_against_row_blocks(dev):
    from gpytorch_amd import backend as B

    ref, V, p1, p2, bound = _case("matern52", 90, 257, 600, 17, dev, ard=True)
    out = _product(p1, p2, V, dev)
    try:
        B.FORCE_CHUNKED = True
        assert not B.fused_f64(p1, p2)
        rows = _product(p1, p2, V, dev)
    finally:
        B.FORCE_CHUNKED = False
    _check(out, rows, bound, 2.0)


def test_slabs_are_reproducible(dev):
    from gpytorch_amd import backend as B

    _, V, p1, p2, _ = _case("rq", 33, 257, 600, 69, dev)
    vt = B.to_probe_major(V.to(dev), torch.float64)
    P, S, ldo = B.kv_partials_f64(p1, p2, vt)
    assert S >= 2
    first = P[: S * 69 * ldo].clone()
    P2, _, _ = B.kv_partials_f64(p1, p2, vt)
    assert torch.equal(first, P2[: S * 69 * ldo])


def test_linear_cg_through_the_hook(dev):
    """float64 mBCG on a d = 40 cloud (kv_partials_hook -> the fused kernel): true residual against the dense float64 system"""
    from gpytorch_amd import backend as B
    from gpytorch_amd.linear_cg import linear_cg

    n, d, t, s2 = 300, 40, 6, 0.05
    g0 = torch.Generator().manual_seed(3)
    X = torch.rand(n, d, generator=g0, dtype=torch.float64)
    rhs = torch.randn(n, t, generator=g0, dtype=torch.float64)
    ls = torch.tensor([0.4 * math.sqrt(d)], dtype=torch.float64)
    A = _cov("rbf", X, X, ls) + s2 * torch.eye(n, dtype=torch.float64)
    xp = B.prep_points("rbf", X.to(dev), ls.to(dev))
    assert B.fused_f64(xp, xp)
    sc = torch.ones(1, dtype=torch.float64, device=dev)
    nz = torch.full((1,), s2, dtype=torch.float64, device=dev)
    sol_t, info = linear_cg(xp, sc, nz, B.to_probe_major(rhs.to(dev), torch.float64), tolerance=1e-4, max_iter=400)
    assert info.tolerance_reached and sol_t.dtype == torch.float64
    res = (A @ B.from_probe_major(sol_t, n).cpu() - rhs).norm(dim=0) / rhs.norm(dim=0)
    assert float(res.mean()) < 1.2e-4
