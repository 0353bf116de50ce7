"""Input gradients of KISS-GP on the device: the derivative-stencil kernel (``backend.ski_interp_grad``) against the float64 restatement
``tests/ski_input_grad_ref.py`` on the same float32 X, G and C; the operator's ``x.grad`` through a product; a deep-kernel model's marginal log
likelihood (the twin of tests/test_gpu_ski.py::test_model_mll with a fixed ``Linear(2, 2)`` in front); eval-mode predictions; three Adam steps of
examples/kissgp_dkl_regression.py.

The kernel's bound.  |got - ref| <= 2^-22 |ref| + 2^-40 A with A = sum_c |C| sum_k |dw| |G|: one float32 rounding of the output, and a float64 sum
whose chain the issue counts flat, 2 t (4^d + 1) <= 2^13 terms of 2^-53 each.  The kernel's own order is nested -- at a node the <= 2 TC columns of a
group, then the four nodes of a row, then the 4^(d-1) rows and the groups -- so every partial sum passes through FEWER additions than the flat
chain, every partial product is bounded by its share of A, and the weights are polynomials of degree three in r evaluated in float64 (a few units
of 2^-53 each): the flat count is an upper bound for this arithmetic too, and the bound stands as stated."""
import functools
import importlib.util
import os
import warnings

import pytest
import torch

from tests import ski_input_grad_ref as GR
from tests import ski_ref as R
from tests.test_gpu_ski import HYP, MODEL_GRID, _data, _grid, _sp

pytestmark = pytest.mark.gpu

TC = 4                         # csrc/kv_ski.hpp SKI_GC
GRIDS = [(4,), (9,), (9, 6), (7, 6, 5), (4, 4, 4)]
NS = [1, 255, 256, 257, 600]   # the edges of the 256-point workgroup
TS = [1, TC - 1, TC, TC + 1, 2 * TC + 3, 11]
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture_points():
    return _load(os.path.join(HERE, "golden", "make_ski_golden.py"), "make_ski_golden_points").points


@functools.lru_cache(maxsize=None)
def _oracle(sizes):
    """Per grid, once: 600 float32 points from the fixture's ``points()`` (interior draws, nodes with r = 0, first- and last-cell points, grid.min and
    grid.max; 40 per call), and per n in NS the float64 dW and boundary mask of the first n."""
    gen = torch.Generator().manual_seed(7000 + sum(sizes) + len(sizes))
    grid = _grid(sizes)
    pts = _fixture_points()
    x = torch.cat([pts(grid, gen, torch.float32) for _ in range(-(-max(NS) // 30))])[: max(NS)].float()
    out = {}
    for n in NS:
        xn = x[-n:].contiguous()                                   # (the tail: grid.min / grid.max close every call's block)
        _, dW, edge = GR.dense_w_dw(xn, grid)
        out[n] = (xn, dW, edge)
    return grid, out, gen


def test_constants_are_the_kernels():
    from gpytorch_amd import backend as B

    assert TC == B.SKI_GC and B.SKI_P == 256


def _padded(v, ld, dev):
    """[t, k] -> [t, ld] on the device with NaN behind column k."""
    out = torch.full((v.shape[0], ld), float("nan"))
    out[:, : v.shape[1]] = v
    return out.to(dev)


@pytest.mark.parametrize("sizes", GRIDS, ids=str)
def test_kernel(sizes, dev):
    from gpytorch_amd import backend as B

    grid, clouds, gen = _oracle(sizes)
    spec = B.SkiGridSpec(grid)
    M = spec.nodes
    worst, worst_const, seen_edge = 0.0, 0.0, False
    for n in NS:
        x, dW, edge = clouds[n]
        cloud = B.SkiCloud(x.to(dev), spec)
        seen_edge |= bool(edge.any()) and bool((~edge).any())
        for t in TS:
            GA, GB = torch.randn(t, M, generator=gen), torch.randn(t, M, generator=gen)
            CA, CB = torch.randn(t, n, generator=gen), torch.randn(t, n, generator=gen)
            ga, gb = _padded(GA, M + 3, dev), _padded(GB, M + 3, dev)
            ca, cb = _padded(CA, B.round_up(n, 4), dev), _padded(CB, B.round_up(n, 4), dev)
            ref1, mag1 = GR.contract(dW, GA, CA)
            ref2, mag2 = GR.contract(dW, GB, CB)
            for two in (False, True):
                ref, mag = (ref1 + ref2, mag1 + mag2) if two else (ref1, mag1)
                for order in (True, False):
                    got = B.ski_interp_grad(cloud, ga, ca, gb if two else None, cb if two else None, cell_order=order)
                    assert got.shape == (n, len(sizes)) and got.dtype == torch.float32
                    got = got.double().cpu()
                    assert torch.isfinite(got).all()
                    excess = (got - ref).abs() - (2.0 ** -22 * ref.abs() + 2.0 ** -40 * mag)
                    worst = max(worst, float(((got - ref).abs() / (2.0 ** -22 * ref.abs() + 2.0 ** -40 * mag).clamp_min(1e-300)).max()))
                    assert float(excess.max()) <= 0.0, (sizes, n, t, two, order, float(excess.max()))
                    assert not got[edge].any()                                 # a boundary axis: exactly zero
            # a constant G: the four derivative weights of an axis sum to zero
            cg = torch.full((t, M), 1.7)
            got = B.ski_interp_grad(cloud, _padded(cg, M + 3, dev), ca).double().cpu()
            _, magc = GR.contract(dW, cg, CA)
            worst_const = max(worst_const, float((got.abs() / (2.0 ** -40 * magc).clamp_min(1e-300)).max()))
            assert bool((got.abs() <= 2.0 ** -40 * magc).all())
    print("ski_interp_grad", sizes, "worst |got - ref| / bound", worst, "constant G: worst |got| / (2^-40 A)", worst_const)
    assert seen_edge and worst <= 1.0


def test_kernel_is_bitwise_reproducible(dev):
    from gpytorch_amd import backend as B

    sizes = (7, 6, 5)
    grid, clouds, gen = _oracle(sizes)
    spec = B.SkiGridSpec(grid)
    x = clouds[600][0].to(dev)
    G, Cc = torch.randn(2, 11, spec.nodes, generator=gen).to(dev), torch.randn(2, 11, 600, generator=gen).to(dev)
    a = B.ski_interp_grad(B.SkiCloud(x, spec), G[0], Cc[0], G[1], Cc[1]).clone()
    b = B.ski_interp_grad(B.SkiCloud(x.clone(), spec), G[0], Cc[0], G[1], Cc[1]).clone()
    c = B.ski_interp_grad(B.SkiCloud(x, spec), G[0], Cc[0], G[1], Cc[1], cell_order=False).clone()
    assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- operator
def _hyper_kernel(g, case, dev):
    """The kernels and grids of tests/test_gpu_ski.py::test_hyper_gradients."""
    d = {"d1_single": 1, "d2_ard_scales": 2, "d3_rq": 3}[case]
    sizes = {1: (64,), 2: (33, 17), 3: (7, 6, 5)}[d]
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
    return d, sizes, kern, inner, base, ls, alpha, inner_v, outer_v


@pytest.mark.parametrize("inputs", ["square", "both", "x2_only"])
@pytest.mark.parametrize("case", ["d1_single", "d2_ard_scales", "d3_rq"])
def test_operator_input_gradients(case, inputs, dev):
    """``(L * (op @ R)).sum().backward()``: ``x.grad`` against the restatement and the hyper-parameter gradients against autograd through ski_ref,
    2e-3 norm-relative (the bound of tests/test_gpu_ski.py::test_hyper_gradients); the operator stays the matrix-free one."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    d, sizes, kern, inner, base, ls, alpha, inner_v, outer_v = _hyper_kernel(g, case, dev)
    gen = torch.Generator().manual_seed(140 + d)
    grid = _grid(sizes)
    n, m = 300, (300 if inputs == "square" else 200)
    x1 = (0.01 + 0.98 * torch.rand(n, d, generator=gen)).float()
    x2 = x1 if inputs == "square" else (0.01 + 0.98 * torch.rand(m, d, generator=gen)).float()
    Lm, Rm = torch.randn(n, 3, generator=gen), torch.randn(m, 3, generator=gen)
    a1 = x1.to(dev).requires_grad_(inputs != "x2_only")
    a2 = a1 if inputs == "square" else x2.to(dev).requires_grad_(True)
    op = kern(a1) if inputs == "square" else kern(a1, a2)
    op = op.evaluate_kernel() if hasattr(op, "evaluate_kernel") else op
    assert isinstance(op, SKIFusedLinearOperator) and op.requires_grad
    obj = (Lm.to(dev) * (op @ Rm.to(dev))).sum()
    obj.backward()
    p = {"ls": torch.tensor(ls, dtype=torch.float64, requires_grad=True)}
    got_h = [base.raw_lengthscale.grad.reshape(-1).double().cpu()]
    if alpha:
        p["alpha"] = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
        got_h.append(base.raw_alpha.grad.reshape(-1).double().cpu())
    if inner_v:
        p["inner"] = torch.tensor(inner_v, dtype=torch.float64, requires_grad=True)
        p["outer"] = torch.tensor(outer_v, dtype=torch.float64, requires_grad=True)
        got_h += [inner.raw_outputscale.grad.reshape(-1).double().cpu(), kern.raw_outputscale.grad.reshape(-1).double().cpu()]
    cols = R.columns("rq" if alpha else "rbf", grid, p["ls"], p.get("inner"), p.get("alpha"))
    ref = (Lm.double() * (R.k_ski(x1, x2, grid, cols, p.get("outer")) @ Rm.double())).sum()
    gref = torch.autograd.grad(ref, list(p.values()))
    want_h = [gv * torch.tensor([_sp(float(v)) for v in pv.detach().reshape(-1)], dtype=torch.float64) for gv, pv in zip(gref, p.values())]
    r1, r2 = GR.bilinear_input_grads(x1, x2, grid, cols, outer_v, Lm, Rm)
    if inputs == "square":
        pairs = [(a1.grad, r1 + r2)]
    elif inputs == "both":
        pairs = [(a1.grad, r1), (a2.grad, r2)]
    else:
        assert a1.grad is None
        pairs = [(a2.grad, r2)]
    e_v = abs(float(obj.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    e_x = [float((a.double().cpu() - b).norm() / b.norm()) for a, b in pairs]
    e_h = [float((a - b.reshape(-1)).norm() / b.norm()) for a, b in zip(got_h, want_h)]
    print("operator input grads", case, inputs, e_v, e_x, e_h)
    assert all(a.shape == b.shape and a.dtype == torch.float32 for a, b in pairs)
    assert e_v <= 2e-3 and max(e_x) <= 2e-3 and max(e_h) <= 2e-3


# ---------------------------------------------------------------------------------------------- model
W_FIXED, B_FIXED = [[0.9, 0.02], [0.02, 0.9]], 0.04


def _dkl_model(g, X, y, dev, detach_features=False):
    class DeepKissGP(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.feature_extractor = torch.nn.Linear(2, 2)
            self.mean_module = g.means.ConstantMean()
            self.covar_module = g.kernels.ScaleKernel(
                g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=list(MODEL_GRID), grid_bounds=[(0.0, 1.0)] * 2))

        def forward(self, x):
            z = self.feature_extractor(x)
            z = z.detach() if detach_features else z
            return g.distributions.MultivariateNormal(self.mean_module(z), self.covar_module(z))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = DeepKissGP(X.to(dev), y.to(dev), lik).to(dev)
    m.covar_module.base_kernel.base_kernel.lengthscale, m.covar_module.outputscale, lik.noise = HYP["ls"], HYP["os"], HYP["noise"]
    with torch.no_grad():
        m.mean_module.constant.fill_(HYP["c"])
        m.feature_extractor.weight.copy_(torch.tensor(W_FIXED))
        m.feature_extractor.bias.fill_(B_FIXED)
    return m, lik


def _features(X):
    """The layer in float32, as the device computes it (exact float32 inputs for the restatement)."""
    return X @ torch.tensor(W_FIXED).T + torch.tensor(B_FIXED)


@functools.lru_cache(maxsize=None)
def _dkl_reference(n):
    X, y = _data(n)
    z = _features(X)
    grid = _grid(MODEL_GRID)
    cols = R.columns("rbf", grid, torch.tensor([HYP["ls"]], dtype=torch.float64))
    val, dz = GR.mll_feature_grads(z, y, grid, cols, HYP["os"], HYP["noise"], HYP["c"])
    return val, torch.cat([(dz.T @ X.double()).reshape(-1), dz.sum(0)])


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
def test_dkl_model_mll(branch, dev):
    """tests/test_gpu_ski.py::test_model_mll with a fixed ``Linear(2, 2)`` in front (n = 900, grid 20 x 20, the same settings, seed and bounds): the
    marginal log likelihood and its gradient with respect to the layer's weight and bias against the float64 dense Cholesky restatement."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    n = 900
    X, y = _data(n)
    z = _features(X)
    assert float(z.min()) >= 0.04 and float(z.max()) <= 0.96
    ref, want = _dkl_reference(n)
    m, lik = _dkl_model(g, X, y, dev)
    assert isinstance(m.covar_module(m.feature_extractor(m.train_inputs[0])), SKIFusedLinearOperator)
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
    got = torch.cat([m.feature_extractor.weight.grad.reshape(-1), m.feature_extractor.bias.grad.reshape(-1)]).double().cpu()
    e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
    print("dkl mll", branch, e_v, e_g, got, want)
    assert e_v < tol_v, (branch, float(val), float(ref))
    assert e_g < tol_g, (branch, got, want)


def test_eval_prediction_ignores_requires_grad(dev):
    """Eval mode, grad mode on: the train and test features require grad.  The prediction is the one of detached features (1e-6); the gradient of a
    prediction with respect to the inputs is not provided."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import InterpolatedPredictionStrategy

    n, ns = 900, 60
    X, y = _data(n + ns)
    out = []
    S = g.settings
    for detach in (False, True):
        m, lik = _dkl_model(g, X[:n], y[:n], dev, detach_features=detach)
        m.eval()
        lik.eval()
        torch.manual_seed(1)
        with warnings.catch_warnings(), S.max_cholesky_size(0), S.eval_cg_tolerance(1e-4), S.max_root_decomposition_size(n), S.min_preconditioning_size(100):
            warnings.simplefilter("ignore")
            pred = lik(m(X[n:].to(dev)))
            out.append((pred.mean.detach().double().cpu(), pred.variance.detach().double().cpu()))
        assert isinstance(m.prediction_strategy, InterpolatedPredictionStrategy)
    (mu_a, var_a), (mu_d, var_d) = out
    e_mu, e_var = float((mu_a - mu_d).abs().max() / mu_d.abs().max()), float((var_a - var_d).abs().max() / var_d.abs().max())
    print("eval with attached features", e_mu, e_var)
    assert e_mu <= 1e-6 and e_var <= 1e-6


def test_example_model_three_adam_steps(dev):
    """examples/kissgp_dkl_regression.py's model at n = 2000: after each of three Adam steps every gradient of the feature extractor is finite and
    not zero, and the covariance is the matrix-free operator."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    ex = _load(os.path.join(os.path.dirname(HERE), "examples", "kissgp_dkl_regression.py"), "kissgp_dkl_regression_example")
    torch.manual_seed(0)
    x, y = ex.make_data(2000)
    x, y = x.to(dev), y.to(dev)
    model, lik = ex.build(x, y)
    model.train()
    lik.train()
    op = model.covar_module(model.scale_to_bounds(model.feature_extractor(x)))
    op = op.evaluate_kernel() if hasattr(op, "evaluate_kernel") else op
    assert isinstance(op, SKIFusedLinearOperator) and op.a1 is not None
    opt = ex.make_optimizer(model, lik)
    mll = g.ExactMarginalLogLikelihood(lik, model)
    for step in range(3):
        loss = ex.train_step(model, lik, mll, opt, x, y)
        assert bool(torch.isfinite(loss))
        for name, prm in model.feature_extractor.named_parameters():
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and bool(prm.grad.abs().max() > 0), (step, name)
