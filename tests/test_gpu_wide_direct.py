"""GPU parity of the fused wide product by direct differences (csrc/kv_wide_direct.hpp): float32 clouds of 33 .. 512 dimensions that the Gram-form wide
kernel does not admit -- an extent beyond its norm rule (RBF, Matern 3/2, 5/2), or Matern 1/2.

Ground truth everywhere: the dense float64 K of ``oracle/kernels.py`` (direct pairwise differences) times V on the CPU, from the very float32 inputs
the device sees.  2e-5 is the bound every split-contraction kernel of the library is held to (tests/test_gpu_wide.py, tests/test_gpu_kv_split.py)."""
import math

import pytest
import torch

from oracle import kernels as OK
from tests.test_gpu_wide import _check_columns, _data as _near_data
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu
BOUND = 2e-5
KINDS = ["rbf", "matern12", "matern32", "matern52"]


def _data(kind, d, n, m, t, dev, ard=False):
    """Matern 1/2: the in-rule cloud of test_gpu_wide.  The others: the same cloud and lengthscales with the common origin moved 20 lengthscales away
    along the diagonal (|z|^2 >= 400 / 2 in prepared coordinates for every point; K does not depend on the origin)."""
    from gpytorch_amd import backend as B

    if kind == "matern12":
        return _near_data(kind, d, n, m, t, dev, ard=ard)
    g0 = torch.Generator().manual_seed(0)
    X1 = torch.rand(n, d, generator=g0).double()
    X2 = X1 if m is None else torch.rand(m, d, generator=g0).double()
    ls = torch.full((d,), math.sqrt(d) / 4)
    if ard:
        ls = ls * (0.8 + 0.4 * torch.rand(d, generator=g0))
    V = torch.randn(X2.shape[0], t, generator=g0).double()
    K = OK.kernel_matrix(kind, X1, X2, ls.double().reshape(1, d), 1.0, x1_eq_x2=False, direct=True)
    shift = (X1.mean(0).float() - 20.0 * ls / math.sqrt(d)).to(dev)
    lsd = ls.to(dev) if ard else ls[:1].to(dev)
    p1 = B.prep_points(kind, X1.float().to(dev), lsd, shift)
    p2 = p1 if m is None else B.prep_points(kind, X2.float().to(dev), lsd, shift)
    assert p1.zmax2 > B.WIDE_MAX_SQNORM
    return p1, p2, V, K


@pytest.mark.parametrize("kind,d,n,m,t,form", [
    ("matern12", 33, 77, 131, 1, ""), ("rbf", 48, 333, 517, 4, ""), ("matern32", 129, 300, None, 5, ""), ("matern52", 512, 333, 517, 32, ""),
    ("matern12", 129, 300, None, 33, ""), ("rbf", 512, 77, 131, 64, ""), ("matern32", 33, 333, 517, 65, ""), ("matern12", 512, 300, None, 70, ""),
    ("matern52", 48, 300, None, 65, ""), ("rbf", 33, 300, None, 70, ""), ("matern12", 48, 300, None, 11, "khat"), ("matern52", 129, 333, 517, 33, "ard")])
def test_products_through_kv(kind, d, n, m, t, form, dev):
    from gpytorch_amd import backend as B

    p1, p2, V, K = _data(kind, d, n, m, t, dev, ard=form == "ard")
    assert B.wide_direct_f32(p1, p2) and not B.wide_f32(p1, p2)
    vt = B.to_probe_major(V.to(dev))
    if form == "khat":   # K^ = s K + sigma^2 I
        sc, nz = torch.tensor([1.7], device=dev), torch.tensor([0.3], device=dev)
        out, ref = B.kv(p1, p2, vt, scale=sc, dscale=nz, vd=vt), 1.7 * (K @ V) + 0.3 * V
    else:
        out, ref = B.kv(p1, p2, vt), K @ V
    _check_columns(B.from_probe_major(out, n), ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [33, 512])
@pytest.mark.parametrize("n", [65, 200])
def test_entries(kind, d, n, dev):
    """V = I_65 (two column tiles and the extra column): the output is K itself, the diagonal of the symmetric case included (S = 0 exactly)."""
    from gpytorch_amd import backend as B

    p1, p2, _, K = _data(kind, d, n, None if n == 65 else 65, 1, dev)
    assert B.wide_direct_f32(p1, p2)
    out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(torch.eye(65, device=dev))), n)
    assert float((out.double().cpu() - K).abs().max()) < BOUND


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [33, 512])
def test_far_from_the_origin(kind, d, dev):
    """test_gpu_wide.py::test_at_the_norm_limit with the four clusters 400 squared (prepared) units from the origin instead of 24: the pairs within
    a cluster are unchanged, the Gram form would be off by about 2^-22 * 400."""
    from gpytorch_amd import backend as B

    n, t = 256, 11
    g0 = torch.Generator().manual_seed(0)
    c = torch.randn(4, d, generator=g0)
    c = c / c.norm(dim=1, keepdim=True) * math.sqrt(400.0)
    Z = c[torch.arange(n) % 4] + torch.randn(n, d, generator=g0) / math.sqrt(d)
    X = (Z / B.prep_coef(kind)).float()
    V = torch.randn(n, t, generator=g0).double()
    K = OK.kernel_matrix(kind, X.double(), X.double(), torch.ones(1, 1, dtype=torch.float64), 1.0, x1_eq_x2=False, direct=True)
    xp = B.prep_points(kind, X.to(dev), torch.ones(1, device=dev))
    assert xp.zmax2 > B.WIDE_MAX_SQNORM and float((K > 0.01).double().mean()) >= 0.2
    assert B.wide_direct_f32(xp, xp) and not B.wide_f32(xp, xp)
    out = B.from_probe_major(B.kv(xp, xp, B.to_probe_major(V.to(dev))), n)
    assert rel_err(out, K @ V) < BOUND


def test_slabs(dev):
    """A plan of several slabs: the partials stay inside the planned workspace, and the reduced product matches."""
    from gpytorch_amd import backend as B

    kind, d, n, m, t = "matern12", 33, 640, 2048, 6
    p1, p2, V, K = _data(kind, d, n, m, t, dev)
    plan = B.WideDirectPlan(p1, p2, t)
    assert plan.S >= 2 and plan.ws >= plan.S * t * plan.ld and plan.P.numel() > plan.ws
    plan.P.fill_(float("nan"))
    out = B.from_probe_major(plan.product(B.to_probe_major(V.to(dev))), n)
    assert bool(torch.isnan(plan.P[plan.ws:]).all())
    assert bool(torch.isfinite(plan.P[: plan.S * t * plan.ld].view(plan.S, t, plan.ld)[:, :, :n]).all())
    _check_columns(out, K @ V)


def _prep40(kind, dtype, ls, dev, d=40):
    from gpytorch_amd import backend as B

    X, _ = make_data(300, d)
    return B.prep_points(kind, X.to(dtype).to(dev), torch.tensor(ls, dtype=dtype), X.mean(0).to(dtype).to(dev), param=2.0 if kind == "rq" else None)


def test_routing(dev):
    """Matern 1/2 and the RBF cloud beyond the norm rule at d = 40 take the direct-difference plan; RQ, float64, d = 32 and WIDE_KV = False do not."""
    from gpytorch_amd import backend as B

    for kind, ls in (("matern12", 1.6), ("rbf", 0.05)):
        xp = _prep40(kind, torch.float32, ls, dev)
        hook = B.kv_partials_hook(xp, 3)
        assert isinstance(hook, B.WideDirectPlan) and not isinstance(hook, B.WidePlan) and not B.wide_f32(xp, xp)
        B.WIDE_KV = False
        try:
            assert not B.wide_direct_f32(xp, xp) and not isinstance(B.kv_partials_hook(xp, 3), B.WideDirectPlan)
        finally:
            B.WIDE_KV = True
    for kind, dtype, d in (("rq", torch.float32, 40), ("matern12", torch.float64, 40), ("matern12", torch.float32, 32)):
        xp = _prep40(kind, dtype, 1.6, dev, d=d)
        assert not B.wide_direct_f32(xp, xp) and not isinstance(B.kv_partials_hook(xp, 3), B.WideDirectPlan)


def test_solve_agrees_with_the_row_block_path(dev):
    """Matern 1/2, d = 40: one mBCG solve on the direct-difference plan against the same solve on the row-block path -- solutions to 5e-3, iteration
    counts within 3 % (the shape and figures of test_gpu_wide.py::test_routing_solve_agrees_with_the_row_block_path)."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.linear_cg import linear_cg

    kind, n, d, s2, t = "matern12", 3000, 40, 0.5, 12
    X, y = make_data(n, d)
    g0 = torch.Generator().manual_seed(3)
    rhs = torch.cat([torch.randn(n, t - 1, generator=g0), y.float().unsqueeze(-1)], -1)
    xp = B.prep_points(kind, X.float().to(dev), torch.tensor(math.sqrt(d) / 4), X.mean(0).float().to(dev))
    sc, nz = torch.ones(1, device=dev), torch.full((1,), s2, device=dev)
    vt = B.to_probe_major(rhs.to(dev))
    assert isinstance(B.kv_partials_hook(xp, t), B.WideDirectPlan)
    sol_w, info_w = linear_cg(xp, sc, nz, vt, n_tridiag=4, tolerance=1e-3, max_iter=300)
    B.WIDE_KV = False
    try:
        sol_c, info_c = linear_cg(xp, sc, nz, vt, n_tridiag=4, tolerance=1e-3, max_iter=300)
    finally:
        B.WIDE_KV = True
    assert rel_err(sol_w[:, :n], sol_c[:, :n]) < 5e-3
    assert abs(info_w.iterations - info_c.iterations) <= 0.03 * max(info_w.iterations, info_c.iterations)


@pytest.mark.parametrize("kind", ["matern12", "rbf"])
def test_public_interface_at_the_default_lengthscale(kind, dev):
    """ScaleKernel(MaternKernel(nu=0.5)) / ScaleKernel(RBFKernel()) as constructed, on a z-scored cloud of 40 dimensions: the operator times V."""
    import gpytorch_amd as g

    n, d, t = 500, 40, 11
    g0 = torch.Generator().manual_seed(5)
    X = torch.randn(n, d, generator=g0)
    X = ((X - X.mean(0)) / X.std(0)).float()
    V = torch.randn(n, t, generator=g0)
    base = g.kernels.MaternKernel(nu=0.5) if kind == "matern12" else g.kernels.RBFKernel()
    kern = g.kernels.ScaleKernel(base).to(dev)
    with torch.no_grad():
        out = kern(X.to(dev)) @ V.to(dev)
        ls = kern.base_kernel.lengthscale.detach().double().cpu().reshape(1, 1)
        K = float(kern.outputscale) * OK.kernel_matrix(kind, X.double(), X.double(), ls, 1.0, x1_eq_x2=False, direct=True)
    assert rel_err(out, K @ V.double()) < BOUND
