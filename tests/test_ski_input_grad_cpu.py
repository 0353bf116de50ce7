"""Input gradients of KISS-GP without a GPU: the Jacobian of the interpolation weights against the reference's own (tests/golden/
ski_input_grad_values.npz, made by executing the reference under autograd), ``gradcheck`` of the dense restatement ``ski.ski_dense``, the float64
formulas of ``tests/ski_input_grad_ref.py`` against autograd, the envelope of ``ski_input_grad_native``, a deep-kernel model on the dense branch and
the new entry point's declaration, binding and argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gpytorch_amd as g
from gpytorch_amd import backend as B
from gpytorch_amd import ski
from gpytorch_amd.kernels import (GridInterpolationKernel, MaternKernel, RBFKernel, RQKernel, ScaleKernel, ski_input_grad_native, ski_native)
from gpytorch_amd.utils.grid import create_grid
from tests import ski_input_grad_ref as GR
from tests import ski_ref as R
from tests.test_ski_cpu import _Fake

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ski_input_grad_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files if k.endswith("_jac")})


def _case(name):
    grid = []
    while f"{name}_grid{len(grid)}" in GOLD.files:
        grid.append(torch.from_numpy(GOLD[f"{name}_grid{len(grid)}"]))
    x, idx = torch.from_numpy(GOLD[f"{name}_x"]), torch.from_numpy(GOLD[f"{name}_idx"])
    val, jac = torch.from_numpy(GOLD[f"{name}_val"]), torch.from_numpy(GOLD[f"{name}_jac"])
    n, d, M = x.shape[0], x.shape[1], math.prod(a.numel() for a in grid)
    # the node-order mapping of tests/test_ski_cpu.py: the golden indices ARE the flat node indices (axis 0 slowest); scatter values and Jacobian
    W = torch.zeros(n, M, dtype=torch.float64).scatter_add_(1, idx, val)
    J = torch.zeros(n, M, d, dtype=torch.float64).scatter_add_(1, idx.unsqueeze(-1).expand(-1, -1, d), jac)
    return grid, x, W, J


def test_fixture_covers_the_cases():
    sizes = {tuple(int(GOLD[f"{c}_grid{i}"].size) for i in range(3) if f"{c}_grid{i}" in GOLD.files) for c in CASES}
    assert sizes == {(9,), (9, 6), (7, 6, 5), (4, 4, 4), (12,)}
    assert all(GOLD[f"{c}_x"].dtype == np.float64 and GOLD[f"{c}_x"].shape[0] <= 40 for c in CASES)


@pytest.mark.parametrize("name", CASES)
def test_weight_jacobian_matches_the_reference(name):
    """d W[p, :] / d x[p, :] of ``ski.interp_dense_w`` under autograd against the reference's, 1e-10 relative to the row's largest entry; an axis on
    which the point takes the boundary rule carries an exact zero; the restatement's dW is held to the same."""
    grid, x, W, J = _case(name)
    n, d = x.shape
    full = torch.autograd.functional.jacobian(lambda z: ski.interp_dense_w(z, grid), x, vectorize=True)      # [n, M, n, d]
    ar = torch.arange(n)
    mine = full[ar, :, ar, :]                                                                     # [n, M, d]
    off = full.clone()
    off[ar, :, ar, :] = 0.0
    assert not off.any()                                                                          # a point moves its own row only
    assert (ski.interp_dense_w(x, grid) - W).abs().max().item() <= 1e-12                          # the values did not change
    Wr, dWr, edge = GR.dense_w_dw(x, grid)
    assert (Wr - W).abs().max().item() <= 1e-12 and torch.equal(edge.any(-1), R.dense_w(x, grid, return_boundary=True)[1])
    assert edge.any() and (~edge).any()
    worst = 0.0
    for got in (mine, dWr.transpose(1, 2)):
        for p in range(n):
            for a in range(d):
                ref = J[p, :, a]
                if edge[p, a]:
                    assert not ref.any() and not got[p, :, a].any()                               # exactly zero, reference and here
                else:
                    assert ref.abs().max() > 0
                    worst = max(worst, float((got[p, :, a] - ref).abs().max() / ref.abs().max()))
    print("jacobian", name, worst)
    assert worst <= 1e-10
    assert mine.sum(1).abs().max().item() <= 1e-10 * J.abs().max().item()                          # the derivative weights of a point sum to zero


def _grid(sizes, dtype=torch.float64):
    return create_grid(list(sizes), [(0.0, 1.0)] * len(sizes), dtype=dtype)


def _safe_points(grid, n, gen):
    """n float64 points at least 0.05 h from every cell edge (and from the mid-cell switch of the one-hot boundary rule): interior cells, and in the
    first rows the first and the last cell of every axis."""
    cols = []
    for a in grid:
        m, h, g0 = a.numel(), float(a[1] - a[0]), float(a[0])
        cell = torch.randint(1, m - 2, (n,), generator=gen).double()
        cell[0], cell[1] = 0.0, m - 2.0                                                           # first and last cell: the boundary rule
        if n > 3:
            cell[2] = 1.0 if m > 4 else cell[2]
        frac = 0.05 + 0.35 * torch.rand(n, generator=gen, dtype=torch.float64) + 0.5 * (torch.rand(n, generator=gen) < 0.5)
        cols.append(g0 + (cell + frac) * h)
    x = torch.stack(cols, dim=-1)
    return x[torch.randperm(n, generator=gen)] if len(grid) > 1 else x


SIZES = {1: (12,), 2: (9, 6), 3: (7, 6, 5)}


def _columns(grid, d):
    return R.columns("rbf", grid, torch.tensor([0.3, 0.5, 0.7][:d], dtype=torch.float64))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_gradcheck_ski_dense(d):
    gen = torch.Generator().manual_seed(60 + d)
    grid = _grid(SIZES[d])
    x1, x2 = _safe_points(grid, 6, gen).requires_grad_(True), _safe_points(grid, 5, gen).requires_grad_(True)
    _, _, edge = GR.dense_w_dw(torch.cat([x1, x2]).detach(), grid)
    assert edge.any() and (~edge).any()
    cols = _columns(grid, d)
    assert torch.autograd.gradcheck(lambda a, b: ski.ski_dense(a, b, grid, cols), (x1, x2), eps=1e-7, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a: ski.ski_dense(a, a, grid, cols), (x1,), eps=1e-7, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a: ski.ski_dense(a, a, grid, cols, diag=True), (x1,), eps=1e-7, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("d", [2, 3])
def test_gradcheck_additive_dense_form(d):
    """K = sum_q W_q T_q W_q^T over d copies of one axis (``additive=True``), and the dimension batch of the kernel itself."""
    gen = torch.Generator().manual_seed(70 + d)
    axis = _grid((11,))[0]
    x1, x2 = _safe_points([axis] * d, 6, gen).requires_grad_(True), _safe_points([axis] * d, 5, gen).requires_grad_(True)
    cols = R.columns("rbf", [axis] * d, torch.tensor([0.3, 0.5, 0.7][:d], dtype=torch.float64))
    assert torch.autograd.gradcheck(lambda a, b: ski.ski_dense(a, b, [axis] * d, cols, additive=True), (x1, x2), eps=1e-7, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a: ski.interp_dense_w(a, [axis] * d, additive=True), (x1,), eps=1e-7, atol=1e-6, rtol=1e-5)
    k = GridInterpolationKernel(RBFKernel(), grid_size=11, num_dims=1, grid_bounds=[(0.0, 1.0)]).double()
    assert torch.autograd.gradcheck(lambda a, b: k.dimension_batch(a, b), (x1, x2), eps=1e-7, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("scaled", [False, True])
def test_restatement_equals_autograd(d, scaled):
    """The formulas of the issue with dense W and dW (tests/ski_input_grad_ref.py) against autograd through ``ski.ski_dense``, 1e-10."""
    gen = torch.Generator().manual_seed(80 + d)
    grid = _grid(SIZES[d])
    n, m, t = 25, 17, 3
    x1 = torch.cat([_safe_points(grid, n - 6, gen), torch.rand(6, d, generator=gen, dtype=torch.float64)]).requires_grad_(True)
    x2 = torch.rand(m, d, generator=gen, dtype=torch.float64).requires_grad_(True)
    L, Rm, Rs = (torch.randn(k, t, generator=gen, dtype=torch.float64) for k in (n, m, n))
    cols = _columns(grid, d)
    s = 0.8 if scaled else None
    K = ski.ski_dense(x1, x2, grid, cols) * (1.0 if s is None else s)
    a1, a2 = torch.autograd.grad((L * (K @ Rm)).sum(), (x1, x2))
    r1, r2 = GR.bilinear_input_grads(x1.detach(), x2.detach(), grid, cols, s, L, Rm)
    Ks = ski.ski_dense(x1, x1, grid, cols) * (1.0 if s is None else s)
    (asq,) = torch.autograd.grad((L * (Ks @ Rs)).sum(), (x1,))
    xd = x1.detach()
    q1, q2 = GR.bilinear_input_grads(xd, xd, grid, cols, s, L, Rs)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in ((a1, r1), (a2, r2), (asq, q1 + q2))]
    print("restatement", d, scaled, errs)
    assert max(errs) <= 1e-10


def test_ski_input_grad_native_envelope():
    """True exactly where ``ski_native`` would be but for ``requires_grad``; ``ski_native`` itself stays False for such inputs."""
    def kern(sizes, base=None):
        return GridInterpolationKernel(RBFKernel() if base is None else base, grid_size=list(sizes), grid_bounds=[(0.0, 1.0)] * len(sizes))

    k2 = kern((9, 6))
    calls = [(k2, ((10, 2),), {}), (k2, ((10, 2), (7, 2)), {}), (kern((8,)), ((10, 1),), {}), (kern((7, 6, 5)), ((10, 3),), {}),
             (k2, ((10, 2),), {"dtype": torch.float64}), (k2, ((3, 10, 2),), {}), (k2, ((10, 2),), {"device": "cpu"}),
             (kern((5, 5, 5, 5)), ((10, 4),), {}), (k2.double(), ((10, 2),), {}), (kern((256, 256, 256)), ((10, 3),), {}),
             (kern((257, 256, 256)), ((10, 3),), {}), (kern((9, 6), RBFKernel() + MaternKernel()), ((10, 2),), {}),
             (kern((9, 6), RBFKernel(batch_shape=torch.Size([2]))), ((10, 2),), {})]
    calls += [(kern((9, 6), base), ((10, 2),), {}) for base in (MaternKernel(nu=1.5), RQKernel(), ScaleKernel(RBFKernel()))]
    seen = set()
    for k, shapes, kw in calls:
        plain = ski_native(k, *[_Fake(s, **kw) for s in shapes])
        seen.add(plain)
        for which in range(len(shapes)):
            fakes = [_Fake(s, requires_grad=(i == which), **kw) for i, s in enumerate(shapes)]
            assert ski_input_grad_native(k, *fakes) == plain
            assert not ski_native(k, *fakes)
        assert ski_input_grad_native(k, *[_Fake(s, **kw) for s in shapes]) == plain
        assert ski_input_grad_native(k, *[_Fake(s, requires_grad=True, **kw) for s in shapes]) == plain
    assert seen == {True, False}
    assert not ski_input_grad_native(k2, _Fake((10, 2), requires_grad=True), last_dim_is_batch=True)
    small = kern((9, 6))
    small.update_grid([small.grid[0], small.grid[1][:3]])
    with pytest.raises(ValueError, match="at least 4"):
        ski_input_grad_native(small, _Fake((10, 2), requires_grad=True))


def test_kernel_on_the_cpu_hands_the_inputs_their_gradient():
    """The case of the issue: the dense branch of a ``GridInterpolationKernel`` is differentiable in x, next to the lengthscale."""
    k = GridInterpolationKernel(RBFKernel(), 16, num_dims=2)
    x = torch.rand(12, 2, generator=torch.Generator().manual_seed(0)).requires_grad_()
    g.to_dense(k(x)).sum().backward()
    assert x.grad is not None and bool(x.grad.abs().max() > 0) and k.base_kernel.raw_lengthscale.grad is not None


HYP = {"ls": 0.3, "os": 1.3, "noise": 0.1, "c": 0.3}


def test_deep_kernel_model_on_the_dense_branch():
    """``Linear(2, 2)`` in front of the kernel, float64, the CPU: the gradient of the marginal log likelihood with respect to the layer against the
    restatement (dense Cholesky, analytic d mll / d K, the formulas with dW, then the chain rule through the layer), 1e-8."""
    gen = torch.Generator().manual_seed(4)
    n = 60
    X = 0.05 + 0.9 * torch.rand(n, 2, generator=gen, dtype=torch.float64)
    y = torch.sin(5.0 * X[:, 0]) * torch.cos(3.0 * X[:, 1]) + 0.3 + 0.2 * torch.randn(n, generator=gen, dtype=torch.float64)
    layer = torch.nn.Linear(2, 2).double()
    with torch.no_grad():
        layer.weight.copy_(torch.tensor([[0.9, 0.02], [0.02, 0.9]], dtype=torch.float64))
        layer.bias.fill_(0.04)

    class DKL(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.feature_extractor = layer
            self.mean_module = g.means.ConstantMean()
            self.covar_module = g.kernels.ScaleKernel(GridInterpolationKernel(RBFKernel(), grid_size=[20, 20], grid_bounds=[(0.0, 1.0)] * 2))

        def forward(self, x):
            z = self.feature_extractor(x)
            return g.distributions.MultivariateNormal(self.mean_module(z), self.covar_module(z))

    lik = g.likelihoods.GaussianLikelihood().double()
    model = DKL(X, y, lik).double()
    model.covar_module.base_kernel.base_kernel.lengthscale, model.covar_module.outputscale, lik.noise = HYP["ls"], HYP["os"], HYP["noise"]
    with torch.no_grad():
        model.mean_module.constant.fill_(HYP["c"])
    model.train()
    lik.train()
    val = g.ExactMarginalLogLikelihood(lik, model)(model(X), y)
    val.backward()
    grid = [a.detach().clone() for a in model.covar_module.base_kernel.grid]      # (the kernel's own nodes: float32 values, widened)
    z = X @ layer.weight.detach().T + layer.bias.detach()
    cols = R.columns("rbf", grid, torch.tensor([HYP["ls"]], dtype=torch.float64))
    ref, dz = GR.mll_feature_grads(z, y, grid, cols, HYP["os"], float(lik.noise.detach()), HYP["c"])
    want_w, want_b = dz.T @ X, dz.sum(0)
    e_v = abs(float(val.detach()) - float(ref))
    e_w = float((layer.weight.grad - want_w).abs().max() / want_w.abs().max())
    e_b = float((layer.bias.grad - want_b).abs().max() / want_b.abs().max())
    print("dkl cpu", e_v, e_w, e_b)
    assert e_v <= 1e-10 and max(e_w, e_b) <= 1e-8


def test_header_declares_and_lib_binds_the_symbol():
    from gpytorch_amd._lib import SIGNATURES, lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpamd.h")).read()
    assert "int gpamd_ski_interp_grad_f32(const float* X, int64_t ldx, int n, int d, const double* g0, const double* h, const int* m," in header
    assert "#define GPAMD_ABI_VERSION 5" in header
    assert len(SIGNATURES["gpamd_ski_interp_grad_f32"][1]) == 18
    h = lib()
    assert h.gpamd_abi_version() == 5 and B.SKI_GC == 4
    raw = ctypes.create_string_buffer(256)
    buf = ctypes.addressof(raw)          # (non-null host address: never dereferenced before the checks)
    dbl, ints = ctypes.c_double * 3, ctypes.c_int * 3
    g0, hh = dbl(0.0, 0.0, 0.0), dbl(0.1, 0.1, 0.1)

    def grad(d=2, m=(9, 6, 5), X=buf, GA=buf, CA=buf, GB=None, CB=None, dX=buf, ldg=54, ldc=12, ldx=2, lddx=2, n=10, t=2):
        return h.gpamd_ski_interp_grad_f32(X, ldx, n, d, g0, hh, ints(*m), None, GA, CA, GB, CB, ldg, ldc, t, dX, lddx, None)

    what = b"ski_interp_grad"
    assert grad(d=0) == -2 and grad(d=4) == -2 and h.gpamd_last_error() == what + b": d must be in 1..3"
    assert grad(m=(9, 3, 5)) == -1 and h.gpamd_last_error() == what + b": every grid axis needs at least 4 nodes"
    assert grad(d=3, m=(257, 256, 256)) == -2 and h.gpamd_last_error() == what + b": the grid has more than 2^24 nodes"
    for kw in ({"X": None}, {"GA": None}, {"CA": None}, {"dX": None}, {"GB": buf}, {"CB": buf}):
        assert grad(**kw) == -1 and h.gpamd_last_error().startswith(what + b": null pointer")
    assert grad(n=0) == -1 and grad(t=0) == -1 and h.gpamd_last_error() == what + b": bad shape"
    assert grad(ldx=1) == -1 and grad(lddx=1) == -1 and b"row strides" in h.gpamd_last_error()
    assert grad(ldg=53) == -1 and grad(ldc=9) == -1 and h.gpamd_last_error().startswith(what + b": leading dimensions")
