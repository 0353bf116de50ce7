"""GPU parity of the fused wide product (csrc/kv_wide.hpp): float32 clouds of 33 .. 512 dimensions, RBF and Matern 3/2, 5/2.

Ground truth everywhere: the dense float64 K of ``oracle/kernels.py`` (direct pairwise differences) times V on the CPU, from the very float32 inputs
the device sees.  2e-5 is the bound every Gram-form kernel of the library is held to (csrc/gram_f16.hpp, tests/test_gpu_kv_split.py)."""
import math
import warnings

import pytest
import torch

from oracle import kernels as OK
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu
BOUND = 2e-5


def _data(kind, d, n, m, t, dev, ard=False, seed=0):
    """U[0, 1]^d clouds shifted by the mean of x1, lengthscale sqrt(d) / 4 (max |z|^2 <= ~4.5 for every d): prepared clouds, V, the float64 K."""
    from gpytorch_amd import backend as B

    g0 = torch.Generator().manual_seed(seed)
    X1 = torch.rand(n, d, generator=g0).double()
    X2 = X1 if m is None else torch.rand(m, d, generator=g0).double()
    ls = torch.full((d,), math.sqrt(d) / 4)
    if ard:
        ls = ls * (0.8 + 0.4 * torch.rand(d, generator=g0))
    V = torch.randn(X2.shape[0], t, generator=g0).double()
    K = OK.kernel_matrix(kind, X1, X2, ls.double().reshape(1, d), 1.0, x1_eq_x2=False, direct=True)
    shift = X1.mean(0).float().to(dev)
    lsd = ls.to(dev) if ard else ls[:1].to(dev)
    p1 = B.prep_points(kind, X1.float().to(dev), lsd, shift)
    p2 = p1 if m is None else B.prep_points(kind, X2.float().to(dev), lsd, shift)
    return p1, p2, V, K


def _check_columns(out, ref):
    assert rel_err(out, ref) < BOUND
    for c in range(ref.shape[1]):
        assert rel_err(out[:, c], ref[:, c]) < BOUND, c


@pytest.mark.parametrize("kind,d,n,m,t,form", [
    ("rbf", 33, 77, 131, 1, ""), ("matern32", 48, 333, 517, 4, ""), ("matern52", 64, 300, None, 5, ""), ("rbf", 65, 333, 517, 32, ""),
    ("matern32", 129, 300, None, 33, ""), ("matern52", 300, 77, 131, 64, ""), ("rbf", 512, 333, 517, 65, ""), ("matern52", 512, 300, None, 70, ""),
    ("matern32", 33, 333, 517, 65, ""), ("rbf", 129, 300, None, 11, "khat"), ("matern52", 48, 333, 517, 33, "ard")])
def test_products_through_kv(kind, d, n, m, t, form, dev):
    from gpytorch_amd import backend as B

    p1, p2, V, K = _data(kind, d, n, m, t, dev, ard=form == "ard")
    assert B.wide_f32(p1, p2) and not p1.fused
    vt = B.to_probe_major(V.to(dev))
    if form == "khat":   # K^ = s K + sigma^2 I
        sc, nz = torch.tensor([1.7], device=dev), torch.tensor([0.3], device=dev)
        out, ref = B.kv(p1, p2, vt, scale=sc, dscale=nz, vd=vt), 1.7 * (K @ V) + 0.3 * V
    else:
        out, ref = B.kv(p1, p2, vt), K @ V
    _check_columns(B.from_probe_major(out, n), ref)


@pytest.mark.parametrize("kind", ["rbf", "matern32", "matern52"])
@pytest.mark.parametrize("d", [33, 512])
@pytest.mark.parametrize("n", [65, 200])
def test_entries(kind, d, n, dev):
    """V = I_65 (two column tiles and the extra column): the output is K itself, the diagonal of the symmetric case included (the clamp at S = 0)."""
    from gpytorch_amd import backend as B

    p1, p2, _, K = _data(kind, d, n, None if n == 65 else 65, 1, dev)
    out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(torch.eye(65, device=dev))), n)
    assert float((out.double().cpu() - K).abs().max()) < BOUND


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [33, 512])
def test_at_the_norm_limit(kind, d, dev):
    """Four clusters 24 squared (prepared) units from the origin, lengthscale 1: nearby pairs sit at |z|^2 = 25 .. 31 -- the cancellation case the
    norm rule exists for."""
    from gpytorch_amd import backend as B

    n, t = 256, 11
    g0 = torch.Generator().manual_seed(0)
    c = torch.randn(4, d, generator=g0)
    c = c / c.norm(dim=1, keepdim=True) * math.sqrt(24.0)
    Z = c[torch.arange(n) % 4] + torch.randn(n, d, generator=g0) / math.sqrt(d)
    X = (Z / B.prep_coef(kind)).float()
    V = torch.randn(n, t, generator=g0).double()
    K = OK.kernel_matrix(kind, X.double(), X.double(), torch.ones(1, 1, dtype=torch.float64), 1.0, x1_eq_x2=False, direct=True)
    xp = B.prep_points(kind, X.to(dev), torch.ones(1, device=dev))
    assert 24.0 < xp.zmax2 <= B.WIDE_MAX_SQNORM and float((K > 0.01).double().mean()) >= 0.2
    assert B.wide_f32(xp, xp)
    out = B.from_probe_major(B.kv(xp, xp, B.to_probe_major(V.to(dev))), n)
    assert rel_err(out, K @ V) < BOUND


def test_slabs(dev):
    """A plan of several slabs: the partials stay inside the planned workspace, and the reduced product matches."""
    from gpytorch_amd import backend as B

    kind, d, n, m, t = "matern32", 33, 640, 2048, 6
    p1, p2, V, K = _data(kind, d, n, m, t, dev)
    plan = B.WidePlan(p1, p2, t)
    assert plan.S >= 2 and plan.ws >= plan.S * t * plan.ld and plan.P.numel() > plan.ws
    plan.P.fill_(float("nan"))
    out = B.from_probe_major(plan.product(B.to_probe_major(V.to(dev))), n)
    assert bool(torch.isnan(plan.P[plan.ws:]).all())
    assert bool(torch.isfinite(plan.P[: plan.S * t * plan.ld].view(plan.S, t, plan.ld)[:, :, :n]).all())
    _check_columns(out, K @ V)


def test_routing_solve_agrees_with_the_row_block_path(dev):
    """d = 40, RBF: the mBCG hook is the wide plan, and the solve agrees with the same solve on the row-block path -- solutions to 5e-3, iteration
    counts within 3 %, the figures of test_gpu_generic.py::test_generic_path_equals_fused_path_on_the_same_problem.
    The noise 0.5 makes the count a property of the problem, not of rounding: the oracle's CG on the CPU (oracle/linear_cg.py on the dense float64 K)
    takes 31 iterations in float64, in float32, and in float32 with K perturbed entry by entry by 1e-6, 5e-6 and 2e-5 relative.  At noise 0.05 the
    same five runs take 50, 58, 61, 62 and 62 -- float32 rounding alone moves that count by more than 3 %, so two correct float32 routes cannot be
    held to the bound there (the device gave 58 and 61)."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.linear_cg import linear_cg

    kind, n, d, s2, t = "rbf", 3000, 40, 0.5, 12
    X, y = make_data(n, d)
    g0 = torch.Generator().manual_seed(3)
    rhs = torch.cat([torch.randn(n, t - 1, generator=g0), y.float().unsqueeze(-1)], -1)
    xp = B.prep_points(kind, X.float().to(dev), torch.tensor(math.sqrt(d) / 4), X.mean(0).float().to(dev))
    sc, nz = torch.ones(1, device=dev), torch.full((1,), s2, device=dev)
    vt = B.to_probe_major(rhs.to(dev))
    assert isinstance(B.kv_partials_hook(xp, t), B.WidePlan)
    sol_w, info_w = linear_cg(xp, sc, nz, vt, n_tridiag=4, tolerance=1e-3, max_iter=300)
    B.WIDE_KV = False
    try:
        assert not isinstance(B.kv_partials_hook(xp, t), B.WidePlan)
        sol_c, info_c = linear_cg(xp, sc, nz, vt, n_tridiag=4, tolerance=1e-3, max_iter=300)
    finally:
        B.WIDE_KV = True
    print("iterations", info_w.iterations, info_c.iterations, "rel_err", rel_err(sol_w[:, :n], sol_c[:, :n]))
    assert rel_err(sol_w[:, :n], sol_c[:, :n]) < 5e-3
    assert abs(info_w.iterations - info_c.iterations) <= 0.03 * max(info_w.iterations, info_c.iterations)


@pytest.mark.parametrize("kind,dtype,ls", [("matern12", torch.float32, 1.6), ("rq", torch.float32, 1.6), ("rbf", torch.float64, 1.6), ("rbf", torch.float32, 0.05)])
def test_routing_keeps_the_row_block_path(kind, dtype, ls, dev):
    """Matern 1/2, RQ, float64 and a cloud beyond the norm rule (max |z|^2 > 32) at d = 40 stay on the chunked route."""
    from gpytorch_amd import backend as B

    X, _ = make_data(300, 40)
    xp = B.prep_points(kind, X.to(dtype).to(dev), torch.tensor(ls, dtype=dtype), X.mean(0).to(dtype).to(dev), param=2.0 if kind == "rq" else None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert not B.wide_f32(xp, xp) and not isinstance(B.kv_partials_hook(xp, 3), B.WidePlan)
    if ls < 1.0:
        assert xp.zmax2 > B.WIDE_MAX_SQNORM
