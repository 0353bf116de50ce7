"""KISS-GP on the device: the gather W U, the scatter W^T V (no atomics) and the full product against the float64 restatement ``tests/ski_ref.py`` on
float32-exact inputs; special clouds (nodes, boundary cells, one long cell, empty cells, coordinates near 1000); bitwise reproducibility; the
operator algebra; hyper-gradients; the axis order under ARD; a model's marginal log likelihood and posterior.

Bounds: products 2e-5 per column relative to the column maximum of |W| K_UU |W|^T |V| (tests/test_gpu_product.py's K V bound; the single stages use
the analogous normaliser), entries 1e-5 max-normalised, hyper-gradients 2e-3, the model's as tests/test_gpu_rbfgrad.py."""
import functools
import math
import warnings

import pytest
import torch

from tests import ski_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

P, G, C = 256, 256, 4          # csrc/kv_ski.hpp SKI_P (gather: points per workgroup), SKI_G (scatter: nodes per workgroup), SKI_C (column group)
GRIDS = [(4,), (5,), (64,), (2000,), (9, 6), (33, 17), (4, 4, 4), (7, 6, 5), (33, 17, 9)]
NS = [1, 7, P - 1, P, P + 1, 3 * P + 5]
TS = [1, 2, C, C + 1, 11]
LS = {1: 0.1, 2: 0.2, 3: 0.35}
TOL = 2e-5


def test_constants_are_the_kernels():
    from gpytorch_amd import backend as B

    assert (P, G, C) == (B.SKI_P, B.SKI_G, B.SKI_C)


def _grid(sizes, bounds=None):
    from gpytorch_amd.utils.grid import create_grid

    return create_grid(list(sizes), [(0.0, 1.0)] * len(sizes) if bounds is None else bounds)


def _inside(grid, n, gen):
    """n uniform float32 points in the interior of the grid: between node 1 and node m - 2 of every axis, where no boundary rule applies."""
    lo = torch.stack([a[1] for a in grid])
    hi = torch.stack([a[-2] for a in grid])
    return (lo + (0.01 + 0.98 * torch.rand(n, len(grid), generator=gen)) * (hi - lo)).float()


@functools.lru_cache(maxsize=None)
def _oracle(sizes):
    """Per grid, computed once and shared by the gather, scatter and product tests: float32 clouds of every size in NS, uniform on [0, 1]^d (the
    grid's bounds: inside the grid, a few points in its first and last cells), their float64 W and boundary masks, and the float64 Toeplitz columns
    of the RBF base kernel."""
    gen = torch.Generator().manual_seed(900 + sum(sizes) + len(sizes))
    grid = _grid(sizes)
    d = len(sizes)
    clouds = {}
    for n in NS:
        x = torch.rand(n, d, generator=gen)
        W, edge = R.dense_w(x, grid, return_boundary=True)
        clouds[n] = (x, W, edge)
    cols = R.columns("rbf", grid, torch.tensor([LS[d]]).float())
    return grid, clouds, cols, gen


def _vectors(gen, t, n):
    return torch.randn(t, n, generator=gen)


def _pm(v, dev):
    """[t, n] -> probe-major [t, ld] on the device."""
    from gpytorch_amd import backend as B

    out = torch.zeros(v.shape[0], B.round_up(v.shape[1], 4))
    out[:, : v.shape[1]] = v
    return out.to(dev)


def _col_err(got, want, norm):
    """max over columns of max|got - want| / norm; got, want [rows, t], norm [t]."""
    return float(((got.double() - want).abs().max(0)[0] / norm.clamp_min(1e-300)).max())


@pytest.mark.parametrize("sizes", GRIDS, ids=str)
def test_gather(sizes, dev):
    from gpytorch_amd import backend as B

    grid, clouds, _, gen = _oracle(sizes)
    spec = B.SkiGridSpec(grid)
    worst = 0.0
    for n in NS:
        x, W, _ = clouds[n]
        cloud = B.SkiCloud(x.to(dev), spec)
        for t in TS:
            U = _vectors(gen, t, spec.nodes)
            out = B.ski_interp(cloud, U.to(dev)).cpu()
            assert out.shape == (t, B.round_up(n, 4)) and not out[:, n:].any()
            worst = max(worst, _col_err(out[:, :n].t(), W @ U.double().t(), (W.abs() @ U.double().abs().t()).max(0)[0]))
    print("gather", sizes, worst)
    assert worst <= TOL


@pytest.mark.parametrize("sizes", GRIDS, ids=str)
def test_scatter(sizes, dev):
    from gpytorch_amd import backend as B

    grid, clouds, _, gen = _oracle(sizes)
    spec = B.SkiGridSpec(grid)
    worst = 0.0
    for n in NS:
        x, W, _ = clouds[n]
        cloud = B.SkiCloud(x.to(dev), spec)
        for t in TS:
            V = _vectors(gen, t, n)
            out = B.ski_interp_t(cloud, _pm(V, dev)).cpu()
            assert out.shape == (t, spec.nodes)
            worst = max(worst, _col_err(out.t(), W.t() @ V.double().t(), (W.abs().t() @ V.double().abs().t()).max(0)[0]))
    print("scatter", sizes, worst)
    assert worst <= TOL


def _kernel(g, sizes, dev, ls=None, bounds=None):
    d = len(sizes)
    k = g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=list(sizes), grid_bounds=[(0.0, 1.0)] * d if bounds is None else bounds).to(dev)
    k.base_kernel.lengthscale = LS[d] if ls is None else ls
    return k


def _product_check(op, x1, W1, x2, W2, cols, gen, t, dev):
    n, m = W1.shape[0], W2.shape[0]
    V = _vectors(gen, t, m)
    with torch.no_grad():
        out = (op @ V.t().contiguous().to(dev)).cpu()
    assert out.shape == (n, t)
    want = W1 @ R.kuu_matmul(cols, W2.t() @ V.double().t())
    norm = (W1.abs() @ R.kuu_matmul([c.abs() for c in cols], W2.abs().t() @ V.double().abs().t())).max(0)[0]
    return _col_err(out, want, norm)


@pytest.mark.parametrize("sizes", GRIDS, ids=str)
def test_product(sizes, dev):
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    grid, clouds, cols, gen = _oracle(sizes)
    k = _kernel(g, sizes, dev)
    worst = 0.0
    for i, n in enumerate(NS):
        m = NS[(i + 2) % len(NS)]                      # a different size for x2
        (x1, W1, _), (x2, W2, _) = clouds[n], clouds[m]
        with torch.no_grad():
            op = k(x1.to(dev), x2.to(dev))
        assert isinstance(op, SKIFusedLinearOperator) and op.shape == (n, m)
        for t in TS:
            worst = max(worst, _product_check(op, x1, W1, x2, W2, cols, gen, t, dev))
    # the test's own inputs are informative: K_ski is neither ~0 nor ~1 everywhere and the stencils carry negative weights, so that neither a
    # missing stencil node nor a swapped axis can pass
    (x1, W1, _), (x2, W2, _) = clouds[NS[-1]], clouds[NS[-2]]
    K = W1 @ R.kuu_matmul(cols, W2.t())
    mid = float(((K > 0.05) & (K < 0.95)).double().mean())
    neg = float((W1 < 0).sum()) / (W1.shape[0] * 4 ** len(sizes))
    print("product", sizes, worst, "share of K in (0.05, 0.95)", mid, "negative weights", neg)
    assert 0.05 <= mid <= 0.95 and neg >= 0.05
    assert worst <= TOL


def _special(kind, sizes, gen):
    grid = _grid(sizes)
    d = len(sizes)
    lo = torch.stack([a[0] for a in grid])
    hi = torch.stack([a[-1] for a in grid])
    h = torch.stack([a[1] - a[0] for a in grid])
    if kind == "nodes":
        x = torch.stack([torch.stack([a[int(torch.randint(0, a.numel(), (1,), generator=gen))] for a in grid]) for _ in range(60)])
    elif kind == "edge":
        x = _inside(grid, 120, gen)
        ax = torch.randint(0, d, (120,), generator=gen)
        side = torch.rand(120, generator=gen) < 0.5
        off = (0.02 + 0.96 * torch.rand(120, generator=gen)) * h[ax]
        x[torch.arange(120), ax] = torch.where(side, lo[ax] + off, hi[ax] - off)
    elif kind == "minmax":
        x = torch.stack([torch.where(torch.tensor([(c >> i) & 1 == 1 for i in range(d)]), hi, lo) for c in range(2 ** d)])
    elif kind == "one_cell":
        x = lo + 2.0 * h + (0.02 + 0.96 * torch.rand(P + 1, d, generator=gen)) * h        # P + 1 points in the cell with stencil base 1
    else:
        raise KeyError(kind)
    return grid, x.float()


@pytest.mark.parametrize("sizes", [(9,), (9, 6), (7, 6, 5)], ids=str)
@pytest.mark.parametrize("kind", ["nodes", "edge", "minmax", "one_cell"])
def test_special_clouds(kind, sizes, dev):
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(77 + len(sizes))
    grid, x = _special(kind, sizes, gen)
    W, edge = R.dense_w(x, grid, return_boundary=True)
    if kind in ("edge", "minmax"):
        assert edge.all()                                                 # every point takes the boundary rule ...
    if kind == "one_cell":
        assert not edge.any()                                             # ... and none of an interior cloud
    x2 = _inside(grid, P - 1, gen)
    W2, e2 = R.dense_w(x2, grid, return_boundary=True)
    assert not e2.any()                                                   # the interior cloud on the other side: 0 % boundary-rule points
    cols = _oracle(sizes)[2]
    spec = B.SkiGridSpec(grid)
    cloud = B.SkiCloud(x.to(dev), spec)
    if kind == "one_cell":
        assert cloud.max_count == P + 1 and cloud.nchunks == 2            # the long list: summed in chunks
    n, t = x.shape[0], C + 1
    U, V = _vectors(gen, t, spec.nodes), _vectors(gen, t, n)
    e_g = _col_err(B.ski_interp(cloud, U.to(dev)).cpu()[:, :n].t(), W @ U.double().t(), (W.abs() @ U.double().abs().t()).max(0)[0])
    e_s = _col_err(B.ski_interp_t(cloud, _pm(V, dev)).cpu().t(), W.t() @ V.double().t(), (W.abs().t() @ V.double().abs().t()).max(0)[0])
    k = _kernel(g, sizes, dev)
    with torch.no_grad():
        e_p = max(_product_check(k(x.to(dev), x2.to(dev)), x, W, x2, W2, cols, gen, t, dev),
                  _product_check(k(x2.to(dev), x.to(dev)), x2, W2, x, W, cols, gen, t, dev),
                  _product_check(k(x.to(dev)), x, W, x, W, cols, gen, 1, dev))
    print("special", kind, sizes, e_g, e_s, e_p)
    assert max(e_g, e_s, e_p) <= TOL


def test_almost_every_cell_empty(dev):
    import gpytorch_amd as g

    sizes = (33, 17, 9)
    gen = torch.Generator().manual_seed(5)
    grid = _grid(sizes)
    x = _inside(grid, 7, gen)
    W = R.dense_w(x, grid)
    cols = _oracle(sizes)[2]
    k = _kernel(g, sizes, dev)
    with torch.no_grad():
        err = _product_check(k(x.to(dev)), x, W, x, W, cols, gen, 11, dev)
    assert err <= TOL


@pytest.mark.parametrize("d", [1, 2])
def test_coordinates_near_1000(d, dev):
    """A cloud and a grid near 1000 with h = 0.02: float32 index arithmetic would lose 1e-4 of a weight here, the float64 arithmetic of the kernels
    does not."""
    import gpytorch_amd as g

    sizes = (50,) * d
    bounds = [(1000.0, 1000.96)] * d
    gen = torch.Generator().manual_seed(11)
    grid = _grid(sizes, bounds)
    x = (1000.0 + 0.01 + 0.94 * torch.rand(300, d, generator=gen)).float()
    W, edge = R.dense_w(x, grid, return_boundary=True)
    assert not edge.any()
    cols = R.columns("rbf", grid, torch.tensor([0.1]).float())
    k = _kernel(g, sizes, dev, ls=0.1, bounds=bounds)
    with torch.no_grad():
        err = _product_check(k(x.to(dev)), x, W, x, W, cols, gen, C + 1, dev)
    print("near 1000", d, err)
    assert err <= TOL


@pytest.mark.parametrize("kind", ["one_cell", "uniform"])
def test_bitwise_reproducible(kind, dev):
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    sizes = (7, 6, 5)
    gen = torch.Generator().manual_seed(3)
    x = _special("one_cell", sizes, gen)[1] if kind == "one_cell" else _oracle(sizes)[1][3 * P + 5][0]
    grid = _grid(sizes)
    V = _vectors(gen, 11, x.shape[0])
    xd, vd = x.to(dev), _pm(V, dev)
    a = B.ski_interp_t(B.SkiCloud(xd, B.SkiGridSpec(grid)), vd).clone()
    b = B.ski_interp_t(B.SkiCloud(xd.clone(), B.SkiGridSpec(grid)), vd).clone()
    assert torch.equal(a, b)
    k = _kernel(g, sizes, dev)
    rhs = V.t().contiguous().to(dev)
    with torch.no_grad():
        p1 = (k(xd) @ rhs).clone()
        p2 = (k(xd.clone()) @ rhs).clone()
    assert torch.equal(p1, p2)


def test_operator_algebra(dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import DiagLinearOperator
    from gpytorch_amd.ski import SKIFusedAddedDiagLinearOperator, SKIFusedLinearOperator

    sizes = (9, 6)
    grid, clouds, cols, gen = _oracle(sizes)
    (x1, W1, _), (x2, W2, _) = clouds[P + 1], clouds[P - 1]
    k = g.kernels.ScaleKernel(_kernel(g, sizes, dev)).to(dev)
    k.outputscale = 1.7
    want = 1.7 * (W1 @ R.k_uu(cols) @ W2.t())
    sq = 1.7 * (W1 @ R.k_uu(cols) @ W1.t())
    tol = 1e-5

    def err(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    with torch.no_grad():
        op = k(x1.to(dev), x2.to(dev))
        assert isinstance(op, SKIFusedLinearOperator) and op.scale is not None
        assert err(op.to_dense(), want) <= tol
        assert err(op @ torch.eye(P - 1, device=dev), want) <= tol
        assert err(op.mT.to_dense(), want.t()) <= tol and err(op.mT @ torch.eye(P + 1, device=dev), want.t()) <= tol
        sub = op[10:60, 5:40]
        assert isinstance(sub, SKIFusedLinearOperator) and err(sub.to_dense(), want[10:60, 5:40]) <= tol
        assert err(sub @ torch.eye(35, device=dev), want[10:60, 5:40]) <= tol
        assert err((op * 2.5).to_dense(), 2.5 * want) <= tol and err((op * 2.5) @ torch.eye(P - 1, device=dev), 2.5 * want) <= tol
        assert err(op.diagonal(), want.diagonal()) <= tol
        sqop = k(x1.to(dev))
        assert err(sqop.diagonal(), sq.diagonal()) <= tol
        assert err(k(x1.to(dev), diag=True), sq.diagonal()) <= tol
        for p in (0, 17, P):
            assert err(sqop._row(torch.tensor([p], device=dev)), sq[p]) <= tol
        dvec = 0.1 + torch.rand(P + 1, generator=gen)
        added = sqop + DiagLinearOperator(dvec.to(dev))
        assert isinstance(added, SKIFusedAddedDiagLinearOperator)
        assert err(added.to_dense(), sq + torch.diag(dvec.double())) <= tol
        assert err(added @ torch.eye(P + 1, device=dev), sq + torch.diag(dvec.double())) <= tol
        assert err(added.diagonal(), sq.diagonal() + dvec.double()) <= tol
        joint = k(torch.cat([x1, x2]).to(dev))[..., P + 1:, : P + 1]        # the slice ExactGP.__call__ takes
        assert isinstance(joint, SKIFusedLinearOperator) and err(joint.to_dense(), want.t()) <= tol


def _sp(v):
    return 1.0 - math.exp(-v)       # d softplus(raw) / d raw at the value v


@pytest.mark.parametrize("case", ["d1_single", "d2_ard_scales", "d3_rq"])
def test_hyper_gradients(case, dev):
    """The gradients of sum_c l_c^T K r_c through the device path against autograd through ski_ref in float64: lengthscale (single, ARD), the outer
    and the inner outputscale, RQ's alpha."""
    import gpytorch_amd as g

    d = {"d1_single": 1, "d2_ard_scales": 2, "d3_rq": 3}[case]
    sizes = {1: (64,), 2: (33, 17), 3: (7, 6, 5)}[d]
    gen = torch.Generator().manual_seed(40 + d)
    grid = _grid(sizes)
    x = (0.01 + 0.98 * torch.rand(300, d, generator=gen)).float()
    Lm, Rm = torch.randn(300, 3, generator=gen), torch.randn(300, 3, generator=gen)
    K = g.kernels
    if case == "d1_single":
        base, ls, alpha = K.RBFKernel(), [0.1], None
    elif case == "d2_ard_scales":
        base, ls, alpha = K.RBFKernel(ard_num_dims=2), [0.15, 0.3], None
    else:
        base, ls, alpha = K.RQKernel(ard_num_dims=3), [0.3, 0.4, 0.5], 1.6
    inner_v, outer_v = (1.3, 0.7) if case != "d1_single" else (None, None)
    inner = K.ScaleKernel(base) if inner_v else base
    kern = K.GridInterpolationKernel(inner, grid_size=list(sizes), grid_bounds=[(0.0, 1.0)] * d)
    kern = (K.ScaleKernel(kern) if outer_v else kern).to(dev)
    base.lengthscale = torch.tensor(ls)
    if alpha:
        base.alpha = alpha
    if inner_v:
        inner.outputscale, kern.outputscale = inner_v, outer_v
    op = kern(x.to(dev))
    obj = (Lm.to(dev) * (op @ Rm.to(dev))).sum()
    obj.backward()
    got = [base.raw_lengthscale.grad.reshape(-1).double().cpu()]
    p = {"ls": torch.tensor(ls, dtype=torch.float64, requires_grad=True)}
    if alpha:
        p["alpha"] = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
        got.append(base.raw_alpha.grad.reshape(-1).double().cpu())
    if inner_v:
        p["inner"] = torch.tensor(inner_v, dtype=torch.float64, requires_grad=True)
        p["outer"] = torch.tensor(outer_v, dtype=torch.float64, requires_grad=True)
        got += [inner.raw_outputscale.grad.reshape(-1).double().cpu(), kern.raw_outputscale.grad.reshape(-1).double().cpu()]
    cols = R.columns("rq" if alpha else "rbf", grid, p["ls"], p.get("inner"), p.get("alpha"))
    ref = (Lm.double() * (R.k_ski(x, x, grid, cols, p.get("outer")) @ Rm.double())).sum()
    gref = torch.autograd.grad(ref, list(p.values()))
    want = [gv * torch.tensor([_sp(float(v)) for v in pv.detach().reshape(-1)], dtype=torch.float64) for gv, pv in zip(gref, p.values())]
    e_v = abs(float(obj.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    errs = [float((a - b.reshape(-1)).norm() / b.norm()) for a, b in zip(got, want)]
    print("hyper", case, e_v, errs)
    assert e_v <= 2e-3 and max(errs) <= 2e-3, (case, got, want)


def test_axis_order_under_ard(dev):
    """Every ARD lengthscale sits on its own axis: the device path approximates the ARD kernel as well as its oracle does, and ten times better than
    it approximates the kernel with the two lengthscales exchanged."""
    import gpytorch_amd as g

    sizes, ls = (40, 24), [0.1, 0.3]
    gen = torch.Generator().manual_seed(8)
    grid = _grid(sizes)
    x = (0.01 + 0.98 * torch.rand(200, 2, generator=gen)).float()
    kern = g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(ard_num_dims=2), grid_size=list(sizes), grid_bounds=[(0.0, 1.0)] * 2).to(dev)
    kern.base_kernel.lengthscale = torch.tensor(ls)
    with torch.no_grad():
        Kd = (kern(x.to(dev)) @ torch.eye(200, device=dev)).double().cpu()

    def rbf(l):
        z = x.double() / torch.tensor(l, dtype=torch.float64)
        return torch.exp(-0.5 * (z.unsqueeze(1) - z.unsqueeze(0)).pow(2).sum(-1))

    Kr = R.k_ski(x, x, grid, R.columns("rbf", grid, torch.tensor(ls).float()))
    e_dev, e_ref, e_swap = float((Kd - rbf(ls)).abs().max()), float((Kr - rbf(ls)).abs().max()), float((Kd - rbf(ls[::-1])).abs().max())
    print("axis order", e_dev, e_ref, e_swap)
    assert e_dev <= 1.5 * e_ref and e_dev <= 0.1 * e_swap


# ---------------------------------------------------------------------------------------------- model
# The hyper-parameters of the model tests of tests/test_gpu_product.py (lengthscale 0.3, outputscale 1.3, noise 0.1), whose bounds these tests take.  They
# matter for the exact posterior variance: a solve that stops at the relative residual tau = eval_cg_tolerance leaves about tau * (prior variance) in
# the quadratic form, i.e. tau * outputscale / (posterior variance + noise) relative to the predictive variance -- 1e-4 * 1.3 / 0.1 = 1.3e-3 here, under
# the 2e-3 bound (a noise of 0.05 under an outputscale of 1.4 gives 2.5e-3 by the same arithmetic, and measured 2.9e-3).
HYP = {"ls": 0.3, "os": 1.3, "noise": 0.1, "c": 0.3}
MODEL_GRID = (20, 20)


def _data(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    X = (0.01 + 0.98 * torch.rand(n, 2, generator=gen)).float()
    y = torch.sin(5.0 * X[:, 0]) * torch.cos(3.0 * X[:, 1]) + 0.3 + 0.2 * torch.randn(n, generator=gen)
    return X, y.float()


def _model(g, X, y, dev):
    class KissGP(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.mean_module = g.means.ConstantMean()
            self.covar_module = g.kernels.ScaleKernel(
                g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=list(MODEL_GRID), grid_bounds=[(0.0, 1.0)] * 2))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = KissGP(X.to(dev), y.to(dev), lik).to(dev)
    m.covar_module.base_kernel.base_kernel.lengthscale, m.covar_module.outputscale, lik.noise = HYP["ls"], HYP["os"], HYP["noise"]
    with torch.no_grad():
        m.mean_module.constant.fill_(HYP["c"])
    return m, lik


@functools.lru_cache(maxsize=None)
def _model_reference(n):
    X, y = _data(n)
    grid = _grid(MODEL_GRID)
    p = [torch.tensor(HYP[k], dtype=torch.float64, requires_grad=True) for k in ("ls", "os", "noise", "c")]
    ref = R.mll(X, y, grid, R.columns("rbf", grid, p[0].reshape(1)), p[1], p[2], p[3])
    return ref.detach(), torch.autograd.grad(ref, p)


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
def test_model_mll(branch, dev):
    """n = 900, d = 2, grid 20 x 20: the marginal log likelihood and its gradients (lengthscale, outputscale, noise, mean constant) against ski_ref's
    dense float64 Cholesky; BBMM is forced by ``max_cholesky_size(0)`` with the row-built preconditioner on and the probes fixed by the seed (not
    ``settings.deterministic_probes``: see tests/test_gpu_rbfgrad.py on preconditioned estimators)."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    n = 900
    X, y = _data(n)
    ref, gref = _model_reference(n)
    m, lik = _model(g, X, y, dev)
    assert isinstance(m.covar_module(m.train_inputs[0]), SKIFusedLinearOperator)
    mll = g.ExactMarginalLogLikelihood(lik, m)
    m.train()
    lik.train()
    S = g.settings
    with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(300), \
            S.max_preconditioner_size(50), S.min_preconditioning_size(100), S.max_lanczos_quadrature_iterations(100):
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        val = mll(m(m.train_inputs[0]), m.train_targets)
        val.backward()
    tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
    got = torch.cat([m.covar_module.base_kernel.base_kernel.raw_lengthscale.grad.reshape(-1), m.covar_module.raw_outputscale.grad.reshape(-1),
                     lik.raw_noise.grad.reshape(-1), m.mean_module.constant.grad.reshape(-1)]).double().cpu()
    want = torch.stack([gref[0] * _sp(HYP["ls"]), gref[1] * _sp(HYP["os"]), gref[2] * _sp(HYP["noise"] - 1e-4), gref[3]])
    e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
    print("mll", branch, e_v, e_g, got, want)
    assert e_v < tol_v, (branch, float(val), float(ref))
    assert e_g < tol_g, (branch, got, want)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_pred_var"])
def test_model_posterior(fast, dev):
    """Posterior mean and variance at 60 test points against ski_ref's dense float64 posterior, through the interpolated prediction strategy (grid
    caches; the bounds of tests/test_gpu_rbfgrad.py)."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import InterpolatedPredictionStrategy

    n, ns = 900, 60
    X, y = _data(n + ns)
    Xt, yt, Xs = X[:n], y[:n], X[n:]
    grid = _grid(MODEL_GRID)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in HYP.items()}
    mu_ref, cov_ref = R.posterior(Xt, yt, Xs, grid, R.columns("rbf", grid, p["ls"].reshape(1)), p["os"], p["noise"], float(p["c"]))
    var_ref = cov_ref.diagonal() + p["noise"]
    m, lik = _model(g, Xt, yt, dev)
    m.eval()
    lik.eval()
    S = g.settings
    torch.manual_seed(1)
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4), \
            S.max_root_decomposition_size(n), S.min_preconditioning_size(100):
        warnings.simplefilter("ignore")
        pred = lik(m(Xs.to(dev)))
        mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
    assert isinstance(m.prediction_strategy, InterpolatedPredictionStrategy)
    e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
    print("posterior fast_pred_var", fast, e_mu, e_var)
    assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)


def test_float64_model_takes_the_dense_branch(dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import DenseLinearOperator

    grid, clouds, cols, _ = _oracle((9, 6))
    x, W, _ = clouds[7]
    k = _kernel(g, (9, 6), dev).double()
    k.base_kernel.lengthscale = LS[2]
    with torch.no_grad():
        op = k(x.double().to(dev))
    assert isinstance(op, DenseLinearOperator)
    want = W @ R.k_uu(R.columns("rbf", [a.double() for a in grid], torch.tensor([LS[2]], dtype=torch.float64))) @ W.t()
    assert float((op.to_dense().cpu() - want).abs().max()) <= 1e-6
