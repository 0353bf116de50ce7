"""Additive KISS-GP on the device (AdditiveStructureKernel over GridInterpolationKernel(num_dims=1); csrc/kv_ski_add.hpp): the gather W_add U, the
scatter W_add^T V (no atomics) and the full product through the C ABI on d INDEPENDENT axes against the float64 restatement
``tests/ski_additive_ref.py`` on float32-exact inputs; special clouds; bitwise reproducibility; the operator algebra; hyper-gradients; a model's
marginal log likelihood and posterior; the reference's own test restated.

Bounds: those of tests/test_gpu_ski.py -- products and single stages 2e-5 per column relative to the column maximum of the absolute-value product,
entries 1e-5 max-normalised, the model's as ``test_model_mll`` / ``test_model_posterior`` there."""
import functools
import warnings

import pytest
import torch

from tests import ski_additive_ref as A
from tests import ski_ref as R
from tests.test_gpu_ski import C, P, TOL, _col_err, _pm, _sp, _vectors
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SKI_LONG = 256
AXES = [(4, 4), (5, 64), (64, 64, 64), (4, 2000, 9), (12,) * 8, (7,) * 16]
NS = [1, 7, P - 1, P, P + 1, 3 * P + 5]
TS = [1, 2, C, C + 1, 11]
LS = 0.2


def test_constants_are_the_kernels():
    from gpytorch_amd import backend as B

    assert (P, C, SKI_LONG) == (B.SKI_P, B.SKI_C, B.SKI_LONG) and (B.SKI_ADD_MIN_DIM, B.SKI_ADD_MAX_DIM) == (2, 16)


def _grid(sizes, bounds=(0.0, 1.0)):
    """d independent one-dimensional axes on the same bounds."""
    from gpytorch_amd.utils.grid import create_grid

    return [create_grid([m], [bounds])[0] for m in sizes]


def _inside(grid, n, gen):
    """n uniform float32 points between node 1 and node m - 2 of every axis, where no boundary rule applies."""
    lo = torch.stack([a[1] for a in grid])
    hi = torch.stack([a[-2] for a in grid])
    return (lo + (0.01 + 0.98 * torch.rand(n, len(grid), generator=gen)) * (hi - lo)).float()


@functools.lru_cache(maxsize=None)
def _oracle(sizes):
    """Per set of axes, computed once and shared by the gather, scatter and product tests: float32 clouds of every size in NS, uniform on [0, 1]^d
    (inside the grid, a few coordinates in first and last cells), their float64 W_add, and the float64 Toeplitz columns of an RBF base kernel."""
    gen = torch.Generator().manual_seed(1900 + sum(sizes) + len(sizes))
    grid = _grid(sizes)
    clouds = {}
    for n in NS:
        x = torch.rand(n, len(sizes), generator=gen)
        clouds[n] = (x, A.dense_w_add(x, grid))
    cols = R.columns("rbf", grid, torch.tensor([LS]).float())
    return grid, clouds, cols, gen


def _spec(grid):
    from gpytorch_amd import backend as B

    return B.SkiGridSpec(grid, additive=True)


@pytest.mark.parametrize("sizes", AXES, ids=str)
def test_gather(sizes, dev):
    from gpytorch_amd import backend as B

    grid, clouds, _, gen = _oracle(sizes)
    spec = _spec(grid)
    assert spec.nodes == sum(sizes) and spec.cells == sum(m - 3 for m in sizes)
    worst = 0.0
    for n in NS:
        x, W = clouds[n]
        cloud = B.SkiCloud(x.to(dev), spec)
        for t in TS:
            U = _vectors(gen, t, spec.nodes)
            out = B.ski_interp(cloud, U.to(dev)).cpu()
            assert out.shape == (t, B.round_up(n, 4)) and not out[:, n:].any()           # the padding columns stay zero
            worst = max(worst, _col_err(out[:, :n].t(), W @ U.double().t(), (W.abs() @ U.double().abs().t()).max(0)[0]))
    print("gather", sizes, worst)
    assert worst <= TOL


@pytest.mark.parametrize("sizes", AXES, ids=str)
def test_scatter(sizes, dev):
    from gpytorch_amd import backend as B

    grid, clouds, _, gen = _oracle(sizes)
    spec = _spec(grid)
    worst = 0.0
    for n in NS:
        x, W = clouds[n]
        cloud = B.SkiCloud(x.to(dev), spec)
        assert cloud.perm.shape == (n * len(sizes),) and cloud.cell_start.shape == (spec.cells + 1,) and int(cloud.cell_start[-1]) == n * len(sizes)
        for t in TS:
            V = _vectors(gen, t, n)
            out = B.ski_interp_t(cloud, _pm(V, dev)).cpu()
            assert out.shape == (t, spec.nodes)
            worst = max(worst, _col_err(out.t(), W.t() @ V.double().t(), (W.abs().t() @ V.double().abs().t()).max(0)[0]))
    print("scatter", sizes, worst)
    assert worst <= TOL


def _operator(x1, x2, grid, cols, dev, scale=None):
    """The operator on d INDEPENDENT axes, one column per axis: what the C ABI takes (the kernels of the package send d copies of one axis)."""
    from gpytorch_amd.ski import SKIFusedLinearOperator

    gd = [a.to(dev) for a in grid]
    x1d = x1.to(dev)
    return SKIFusedLinearOperator(x1d, x1d if x2 is x1 else x2.to(dev), gd, [c.float().to(dev) for c in cols], scale=scale, spec=_spec(grid))


def _product_check(op, W1, W2, cols, sizes, gen, t, dev):
    n, m = W1.shape[0], W2.shape[0]
    V = _vectors(gen, t, m)
    with torch.no_grad():
        out = (op @ V.t().contiguous().to(dev)).cpu()
    assert out.shape == (n, t)
    want = W1 @ A.kuu_add_matmul(cols, sizes, W2.t() @ V.double().t())
    norm = (W1.abs() @ A.kuu_add_matmul([c.abs() for c in cols], sizes, W2.abs().t() @ V.double().abs().t())).max(0)[0]
    return _col_err(out, want, norm)


@pytest.mark.parametrize("sizes", AXES, ids=str)
def test_product(sizes, dev):
    grid, clouds, cols, gen = _oracle(sizes)
    worst = 0.0
    for i, n in enumerate(NS):
        m = NS[(i + 2) % len(NS)]                      # a different size for x2
        (x1, W1), (x2, W2) = clouds[n], clouds[m]
        op = _operator(x1, x2, grid, cols, dev)
        assert op.shape == (n, m)
        for t in TS:
            worst = max(worst, _product_check(op, W1, W2, cols, sizes, gen, t, dev))
    (x1, W1), (x2, W2) = clouds[NS[-1]], clouds[NS[-2]]
    K = W1 @ A.kuu_add_matmul(cols, sizes, W2.t())
    mid = float(((K > 0.05 * len(sizes)) & (K < 0.95 * len(sizes))).double().mean())
    neg = float((W1 < 0).sum()) / (W1.shape[0] * 4 * len(sizes))
    print("product", sizes, worst, "share of K in (0.05 d, 0.95 d)", mid, "negative weights", neg)
    assert mid >= 0.05 and neg >= 0.05                 # informative inputs: K is not flat and the stencils carry negative weights
    assert worst <= TOL


def _special(kind, gen):
    """(grid sizes, bounds, cloud) of the special clouds."""
    bounds = (0.0, 1.0)
    sizes = (9, 6, 7)
    if kind == "near_1000":
        sizes, bounds = (50, 50), (1000.0, 1000.96)
    elif kind == "long_and_none":
        sizes = (4, 2000)                              # axis 0: ONE cell, long; axis 1: 1997 cells, none long
    elif kind == "exact_long":
        sizes = (6, 6)
    elif kind == "mostly_empty":
        sizes = (2000, 2000)
    grid = _grid(sizes, bounds)
    d = len(sizes)
    lo = torch.stack([a[0] for a in grid])
    hi = torch.stack([a[-1] for a in grid])
    h = torch.stack([a[1] - a[0] for a in grid])
    if kind == "nodes":
        x = torch.stack([torch.stack([a[int(torch.randint(0, a.numel(), (1,), generator=gen))] for a in grid]) for _ in range(60)])
    elif kind == "first_cell":
        x = lo + (0.02 + 0.96 * torch.rand(120, d, generator=gen)) * h
    elif kind == "last_cell":
        x = hi - (0.02 + 0.96 * torch.rand(120, d, generator=gen)) * h
    elif kind == "minmax":
        x = torch.stack([torch.where(torch.tensor([(c >> i) & 1 == 1 for i in range(d)]), hi, lo) for c in range(2 ** d)])
    elif kind == "one_cell":
        x = lo + 2.0 * h + (0.02 + 0.96 * torch.rand(P + 1, d, generator=gen)) * h        # P + 1 points in the cell with stencil base 1, every axis
    elif kind == "duplicates":
        x = _inside(grid, 40, gen)[torch.randint(0, 40, (300,), generator=gen)]
    elif kind == "long_and_none":
        x = _inside(grid, P + 1, gen)
    elif kind == "exact_long":                         # axis 0: exactly SKI_LONG points in the cell of base 1, SKI_LONG + 1 in the cell of base 2
        x = _inside(grid, 2 * SKI_LONG + 1, gen)
        base = torch.cat([torch.full((SKI_LONG,), 2.0), torch.full((SKI_LONG + 1,), 3.0)])[torch.randperm(2 * SKI_LONG + 1, generator=gen)]
        x[:, 0] = lo[0] + (base + 0.02 + 0.96 * torch.rand(2 * SKI_LONG + 1, generator=gen)) * h[0]
    elif kind == "mostly_empty":
        x = _inside(grid, 7, gen)
    elif kind == "near_1000":
        x = 1000.0 + 0.01 + 0.94 * torch.rand(300, d, generator=gen)
    else:
        raise KeyError(kind)
    return sizes, grid, x.float()


SPECIAL = ["nodes", "first_cell", "last_cell", "minmax", "one_cell", "duplicates", "long_and_none", "exact_long", "mostly_empty", "near_1000"]


@pytest.mark.parametrize("kind", SPECIAL)
def test_special_clouds(kind, dev):
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(177)
    sizes, grid, x = _special(kind, gen)
    d = len(sizes)
    W, edge = A.dense_w_add(x, grid, return_boundary=True)
    if kind in ("first_cell", "last_cell", "minmax"):
        assert edge.all()                                                 # every coordinate takes the boundary rule (one-hot weights) ...
    if kind in ("one_cell", "near_1000"):
        assert not edge.any()                                             # ... and none of an interior cloud
    x2 = _inside(grid, P - 1, gen)
    W2, e2 = A.dense_w_add(x2, grid, return_boundary=True)
    assert not e2.any()
    cols = R.columns("rbf", grid, torch.tensor([0.1 * float(grid[0][-1] - grid[0][0])]).float())
    spec = _spec(grid)
    cloud = B.SkiCloud(x.to(dev), spec)
    counts = (cloud.cell_start[1:] - cloud.cell_start[:-1]).cpu()
    if kind == "one_cell":
        assert cloud.max_count == P + 1 and cloud.nchunks == 2 * d        # one long list per axis: summed in chunks
    if kind == "long_and_none":
        assert int(counts[0]) == P + 1 and int(counts[1:].max()) <= SKI_LONG and cloud.nchunks == 2
    if kind == "exact_long":
        assert counts[:3].tolist() == [0, SKI_LONG, SKI_LONG + 1] and int(cloud.chunk_off[2]) == 0 and int(cloud.chunk_off[3]) == 2
    if kind == "mostly_empty":
        assert int((counts == 0).sum()) >= spec.cells - 14
    n, t = x.shape[0], C + 1
    U, V = _vectors(gen, t, spec.nodes), _vectors(gen, t, n)
    e_g = _col_err(B.ski_interp(cloud, U.to(dev)).cpu()[:, :n].t(), W @ U.double().t(), (W.abs() @ U.double().abs().t()).max(0)[0])
    e_s = _col_err(B.ski_interp_t(cloud, _pm(V, dev)).cpu().t(), W.t() @ V.double().t(), (W.abs().t() @ V.double().abs().t()).max(0)[0])
    e_p = max(_product_check(_operator(x, x2, grid, cols, dev), W, W2, cols, sizes, gen, t, dev),
              _product_check(_operator(x2, x, grid, cols, dev), W2, W, cols, sizes, gen, t, dev),
              _product_check(_operator(x, x, grid, cols, dev), W, W, cols, sizes, gen, 1, dev))
    print("special", kind, sizes, e_g, e_s, e_p)
    assert max(e_g, e_s, e_p) <= TOL


@pytest.mark.parametrize("kind", ["one_cell", "uniform"])
def test_bitwise_reproducible(kind, dev):
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(3)
    if kind == "one_cell":
        sizes, grid, x = _special("one_cell", gen)
    else:
        sizes = (12,) * 8
        grid, x = _grid(sizes), _oracle(sizes)[1][3 * P + 5][0]
    cols = R.columns("rbf", grid, torch.tensor([LS]).float())
    V = _vectors(gen, 11, x.shape[0])
    xd, vd = x.to(dev), _pm(V, dev)
    a = B.ski_interp_t(B.SkiCloud(xd, _spec(grid)), vd).clone()
    b = B.ski_interp_t(B.SkiCloud(xd.clone(), _spec(grid)), vd).clone()
    assert torch.equal(a, b)
    rhs = V.t().contiguous().to(dev)
    with torch.no_grad():
        p1 = (_operator(x, x, grid, cols, dev) @ rhs).clone()
        p2 = (_operator(x.clone(), x, grid, cols, dev) @ rhs).clone()
    assert torch.equal(p1, p2)


# ---------------------------------------------------------------------------------------------- the kernels of the package
def _kernel(g, dev, d, m, base=None, inner=False, outer=False, bounds=(0.0, 1.0)):
    """AdditiveStructureKernel over GridInterpolationKernel(num_dims=1), as the reference's test model composes it."""
    K = g.kernels
    base = K.RBFKernel() if base is None else base
    gk = K.GridInterpolationKernel(K.ScaleKernel(base) if inner else base, grid_size=m, num_dims=1, grid_bounds=None if bounds is None else [bounds])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ak = K.AdditiveStructureKernel(K.ScaleKernel(gk) if outer else gk, num_dims=d)
    return ak.to(dev), gk, base


def test_operator_algebra(dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import DiagLinearOperator
    from gpytorch_amd.ski import SKIFusedAddedDiagLinearOperator, SKIFusedLinearOperator

    d, m = 3, 9
    gen = torch.Generator().manual_seed(21)
    x1, x2 = torch.rand(P + 1, d, generator=gen), torch.rand(P - 1, d, generator=gen)
    k, gk, base = _kernel(g, dev, d, m, outer=True)
    base.lengthscale = LS
    k.base_kernel.outputscale = 1.7
    grid = [gk.grid[0].cpu()] * d
    cols = R.columns("rbf", grid[:1], torch.tensor([LS]).float())
    want = 1.7 * A.k_ski_add(x1, x2, grid, cols)
    sq = 1.7 * A.k_ski_add(x1, x1, grid, cols)
    tol = 1e-5

    def err(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert g.kernels.ski_additive_native(k, x1.to(dev), x2.to(dev))
        op = k(x1.to(dev), x2.to(dev))
        assert isinstance(op, SKIFusedLinearOperator) and op.scale is not None and op.spec.additive and op.spec.nodes == d * m
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
        noisy = sqop + DiagLinearOperator(torch.full((P + 1,), 0.3, device=dev))
        assert isinstance(noisy, SKIFusedAddedDiagLinearOperator)
        assert err(noisy @ torch.eye(P + 1, device=dev), sq + 0.3 * torch.eye(P + 1, dtype=torch.float64)) <= tol
        dvec = 0.1 + torch.rand(P + 1, generator=gen)
        added = sqop + DiagLinearOperator(dvec.to(dev))
        assert isinstance(added, SKIFusedAddedDiagLinearOperator)
        assert err(added.to_dense(), sq + torch.diag(dvec.double())) <= tol
        assert err(added @ torch.eye(P + 1, device=dev), sq + torch.diag(dvec.double())) <= tol
        assert err(added.diagonal(), sq.diagonal() + dvec.double()) <= tol
        joint = k(torch.cat([x1, x2]).to(dev))[..., P + 1:, : P + 1]        # the rectangular test x train block ExactGP.__call__ slices
        assert isinstance(joint, SKIFusedLinearOperator) and err(joint.to_dense(), want.t()) <= tol
        assert err(joint @ torch.eye(P + 1, device=dev), want.t()) <= tol


# ---------------------------------------------------------------------------------------------- model
# Hyper-parameters: tests/test_gpu_ski.py's (lengthscale 0.3, noise 0.1) with the PRIOR VARIANCE of its model, 1.3, which is what the bound on the
# exact posterior variance there is derived from (tau * prior variance / noise = 1.3e-3 < 2e-3): an additive kernel has prior variance d * outputscale
# products, so the outputscales below multiply to 1.3 / d.
NOISE = 0.1
M_GRID = 20


def _lattice(n):
    """The reference test's data (test_kissgp_additive_regression.py): an n x n lattice on [0, 1]^2, y = sin(x0) + cos(x1) + noise / 20."""
    t = torch.arange(n, dtype=torch.float32) / (n - 1)
    X = torch.stack([t.repeat_interleave(n), t.repeat(n)], dim=-1)
    y = torch.sin(X[:, 0]) + torch.cos(X[:, 1])
    return X, y


def _data(d):
    gen = torch.Generator().manual_seed(60 + d)
    if d == 2:
        X, y = _lattice(20)
        Xs = torch.rand(60, 2, generator=gen)
        return X, (y + torch.randn(400, generator=gen) / 20.0).float(), Xs.float()
    X = torch.rand(360, d, generator=gen).float()
    y = torch.sin(3.0 * X).sum(-1) + 0.2 * torch.randn(360, generator=gen)
    return X[:300], y[:300].float(), X[300:]


CASES = {  # base family, lengthscales per d, inner outputscale, outer outputscale (as fractions of the prior variance 1.3 / d), alpha
    "single": ("rbf", False, False, False),
    "ard": ("rbf", True, True, False),
    "scales": ("rbf", False, True, True),
    "rq": ("rq", False, True, False),
}


def _values(case, d):
    kind, ard, inner, outer = CASES[case]
    ls = [0.3 + 0.15 * q for q in range(d)] if ard else [0.3]
    total = 1.3 / d
    inner_v, outer_v = (None, None)
    if inner and outer:
        inner_v, outer_v = 1.3, total / 1.3
    elif inner:
        inner_v = total
    return kind, ls, inner_v, outer_v, (1.6 if kind == "rq" else None)


def _model(g, X, y, dev, case, d):
    kind, ls, inner_v, outer_v, alpha = _values(case, d)
    K = g.kernels
    base = (K.RQKernel if kind == "rq" else K.RBFKernel)(ard_num_dims=d if len(ls) > 1 else None)

    class AdditiveKissGP(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module, self.grid_kernel, _ = _kernel(g, dev, d, M_GRID, base, inner=inner_v is not None, outer=outer_v is not None, bounds=None)

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = AdditiveKissGP(X.to(dev), y.to(dev), lik).to(dev)
    base.lengthscale = torch.tensor(ls)
    lik.noise = NOISE
    params = [base.raw_lengthscale]
    if alpha:
        base.alpha = alpha
        params.append(base.raw_alpha)
    if inner_v is not None:
        m.grid_kernel.base_kernel.outputscale = inner_v
        params.append(m.grid_kernel.base_kernel.raw_outputscale)
    if outer_v is not None:
        m.covar_module.base_kernel.outputscale = outer_v
        params.append(m.covar_module.base_kernel.raw_outputscale)
    params.append(lik.raw_noise)
    return m, lik, params


def _oracle_columns(case, d, axis, p):
    kind, _, inner_v, outer_v, alpha = _values(case, d)
    n_ls = len(_values(case, d)[1])
    it = iter(p)
    ls = next(it)
    a = next(it) if alpha else None
    inner = next(it) if inner_v is not None else None
    outer = next(it) if outer_v is not None else None
    noise = next(it)
    cols = R.columns(kind, [axis] * (d if n_ls > 1 else 1), ls, inner, a)
    return cols, outer, noise


def _oracle_params(case, d):
    kind, ls, inner_v, outer_v, alpha = _values(case, d)
    vals = [torch.tensor(ls, dtype=torch.float64)]
    if alpha:
        vals.append(torch.tensor(alpha, dtype=torch.float64))
    vals += [torch.tensor(v, dtype=torch.float64) for v in (inner_v, outer_v) if v is not None]
    vals.append(torch.tensor(NOISE, dtype=torch.float64))
    return [v.requires_grad_(True) for v in vals]


def _chain(p):
    """d softplus(raw) / d raw at every value (the noise constraint's lower bound 1e-4 is the last entry's)."""
    fac = [torch.tensor([_sp(float(v)) for v in pv.detach().reshape(-1)], dtype=torch.float64) for pv in p[:-1]]
    return fac + [torch.tensor([_sp(NOISE - 1e-4)], dtype=torch.float64)]


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
@pytest.mark.parametrize("case,d", [("single", 2), ("ard", 2), ("scales", 2), ("rq", 2), ("ard", 5)])
def test_model_mll_and_hyper_gradients(case, d, branch, dev):
    """The marginal log likelihood and the gradient of every hyper-parameter (a single lengthscale; one lengthscale per input dimension; the inner
    and the outer outputscale; RQ's alpha; the noise) against float64 autograd through the oracle's dense Cholesky.  d = 2: the reference test's
    20 x 20 lattice; d = 5: 300 random points; m = 20.  Settings and tolerances: tests/test_gpu_ski.py::test_model_mll."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    X, y, _ = _data(d)
    m, lik, params = _model(g, X, y, dev, case, d)
    mll = g.ExactMarginalLogLikelihood(lik, m)
    m.train()
    lik.train()
    S = g.settings
    with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(300), \
            S.max_preconditioner_size(50), S.min_preconditioning_size(100), S.max_lanczos_quadrature_iterations(100):
        warnings.simplefilter("ignore")
        assert isinstance(m.covar_module(m.train_inputs[0]), SKIFusedLinearOperator)
        torch.manual_seed(0)
        val = mll(m(m.train_inputs[0]), m.train_targets)
        val.backward()
    axis = m.grid_kernel.grid[0].cpu()
    p = _oracle_params(case, d)
    cols, outer, noise = _oracle_columns(case, d, axis, p)
    ref = A.mll(X, y, [axis] * d, cols, outer, noise)
    gref = torch.autograd.grad(ref, p)
    want = torch.cat([gv.reshape(-1) * f for gv, f in zip(gref, _chain(p))])
    got = torch.cat([q.grad.reshape(-1) for q in params]).double().cpu()
    tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
    e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
    print("mll", case, d, branch, e_v, e_g, got, want)
    assert bool((got != 0).all())
    assert e_v < tol_v, (case, branch, float(val), float(ref))
    assert e_g < tol_g, (case, branch, got, want)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_pred_var"])
@pytest.mark.parametrize("d", [2, 5])
def test_model_posterior(d, fast, dev):
    """Posterior mean and variance at 60 test points against the oracle's dense float64 posterior, through the interpolated prediction strategy
    (grid caches of sum m_q = d m entries); settings and bounds: tests/test_gpu_ski.py::test_model_posterior."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import InterpolatedPredictionStrategy

    X, y, Xs = _data(d)
    n = X.shape[0]
    m, lik, _ = _model(g, X, y, dev, "ard", d)
    m.eval()
    lik.eval()
    S = g.settings
    torch.manual_seed(1)
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4), \
            S.max_root_decomposition_size(n), S.min_preconditioning_size(100):
        warnings.simplefilter("ignore")
        m.covar_module(torch.cat([X, Xs]).to(dev))                    # (the dynamic grid is fitted to train and test points pooled, once)
        pred = lik(m(Xs.to(dev)))
        mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
    assert isinstance(m.prediction_strategy, InterpolatedPredictionStrategy)
    if fast:
        assert m.prediction_strategy.grid_covar_cache.shape[-1] == d * M_GRID
    assert m.prediction_strategy.grid_mean_cache.shape[-1] == d * M_GRID
    axis = m.grid_kernel.grid[0].cpu()
    p = [v.detach() for v in _oracle_params("ard", d)]
    cols, outer, noise = _oracle_columns("ard", d, axis, p)
    mu_ref, cov_ref = A.posterior(X, y, Xs, [axis] * d, cols, outer, noise)
    var_ref = cov_ref.diagonal() + noise
    e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
    print("posterior", d, "fast_pred_var", fast, e_mu, e_var)
    assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)


def test_reference_test_restated(dev):
    """test/examples/test_kissgp_additive_regression.py: the model as the test writes it (ScaleKernel(RBFKernel(ard_num_dims=2)) under
    GridInterpolationKernel(grid_size=100, num_dims=1) under AdditiveStructureKernel(num_dims=2)), 15 Adam steps at lr 0.01 under
    max_preconditioner_size(10), max_cg_iterations(50) and fast_pred_var; every parameter gets a non-zero gradient at every step and the mean
    absolute error on the 10 x 10 test lattice is below 0.2, the reference's own bar."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    torch.manual_seed(1)
    train_x, train_y = _lattice(20)
    train_y = train_y + torch.randn_like(train_y).div_(20.0)
    test_x, test_y = _lattice(10)
    K = g.kernels

    class GPRegressionModel(g.models.ExactGP):
        def __init__(self, train_x, train_y, likelihood):
            super().__init__(train_x, train_y, likelihood)
            self.mean_module = g.means.ZeroMean()
            self.base_covar_module = K.ScaleKernel(K.RBFKernel(ard_num_dims=2))
            self.covar_module = K.AdditiveStructureKernel(K.GridInterpolationKernel(self.base_covar_module, grid_size=100, num_dims=1), num_dims=2)

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        likelihood = g.likelihoods.GaussianLikelihood().to(dev)
        gp_model = GPRegressionModel(train_x.to(dev), train_y.to(dev), likelihood).to(dev)
        mll = g.ExactMarginalLogLikelihood(likelihood, gp_model)
        with g.settings.max_preconditioner_size(10), g.settings.max_cg_iterations(50), g.settings.fast_pred_var():
            gp_model.train()
            likelihood.train()
            assert isinstance(gp_model.covar_module(train_x.to(dev)), SKIFusedLinearOperator)
            optimizer = torch.optim.Adam(gp_model.parameters(), lr=0.01)
            for _ in range(15):
                optimizer.zero_grad()
                loss = -mll(gp_model(train_x.to(dev)), train_y.to(dev))
                loss.backward()
                optimizer.step()
                for param in gp_model.parameters():
                    assert param.grad is not None and param.grad.norm().item() > 0
            gp_model.eval()
            likelihood.eval()
            with torch.no_grad():
                test_preds = likelihood(gp_model(test_x.to(dev))).mean
    mae = float(torch.mean(torch.abs(test_y.to(dev) - test_preds)))
    print("reference test: mean absolute error", mae)
    assert mae < 0.2


def test_float64_model_takes_the_dense_branch(dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import DenseLinearOperator

    d, m = 3, 9
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(7, d, generator=gen, dtype=torch.float64)
    k, gk, base = _kernel(g, dev, d, m)
    k = k.double()
    base.lengthscale = LS
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not g.kernels.ski_additive_native(k, x.to(dev))
        op = k(x.to(dev))
    assert isinstance(op, DenseLinearOperator)
    axis = gk.grid[0].cpu().double()
    want = A.k_ski_add(x, x, [axis] * d, R.columns("rbf", [axis], torch.tensor([LS], dtype=torch.float64)))
    assert float((op.to_dense().cpu() - want).abs().max()) <= 1e-6
