"""KISS-GP (GridInterpolationKernel) without a GPU: the interpolation rule against the reference's own outputs (tests/golden/ski_values.npz, made by
executing the reference), the grid helpers, the reference's ``test_standard`` on the dense path, the gradient assembly through the Toeplitz columns,
the native envelope and the argument checks of the new entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gpytorch_amd
from gpytorch_amd import backend as B
from gpytorch_amd import ski
from gpytorch_amd.kernels import GridInterpolationKernel, MaternKernel, RBFKernel, RQKernel, ScaleKernel, ski_native
from gpytorch_amd.utils.grid import ScaleToBounds, choose_grid_size, create_data_from_grid, create_grid
from tests import ski_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ski_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files if k.endswith("_val")})


def _case(name):
    grid = []
    while f"{name}_grid{len(grid)}" in GOLD.files:
        grid.append(torch.from_numpy(GOLD[f"{name}_grid{len(grid)}"]))
    x = torch.from_numpy(GOLD[f"{name}_x"])
    idx, val = torch.from_numpy(GOLD[f"{name}_idx"]), torch.from_numpy(GOLD[f"{name}_val"])
    W = torch.zeros(x.shape[0], math.prod(g.numel() for g in grid), dtype=val.dtype).scatter_add_(1, idx, val)
    return grid, x, W


def test_fixture_covers_the_cases():
    sizes = {tuple(int(GOLD[f"{c}_grid{i}"].size) for i in range(3) if f"{c}_grid{i}" in GOLD.files) for c in CASES}
    assert {(9,), (9, 6), (7, 6, 5), (4, 4, 4)} <= sizes
    assert {GOLD[f"{c}_x"].dtype for c in CASES} == {np.dtype("float32"), np.dtype("float64")}
    assert all(GOLD[f"{c}_x"].shape[0] <= 40 for c in CASES)


@pytest.mark.parametrize("name", CASES)
def test_interpolation_matches_the_reference(name):
    grid, x, W = _case(name)
    tol = 1e-12 if x.dtype == torch.float64 else 1e-6      # (float32 cases: the reference's own float32 index arithmetic is what is allowed for)
    Wr, edge = R.dense_w(x, grid, return_boundary=True)
    assert (Wr - W.double()).abs().max().item() <= tol
    Wd = ski.interp_dense_w(x, grid)
    assert Wd.dtype == x.dtype and (Wd.double() - W.double()).abs().max().item() <= tol
    assert edge.any() and (W < 0).any()                     # boundary-rule points and negative weights are both present
    # ski_dense with identity Toeplitz columns (T_i = I) is W_1 W_2^T
    cols = [torch.zeros(g.numel(), dtype=x.dtype).index_fill_(0, torch.tensor([0]), 1.0) for g in grid]
    K = ski.ski_dense(x, x[:7], grid, cols)
    assert (K.double() - (W @ W[:7].T).double()).abs().max().item() <= 10 * tol
    assert (ski.ski_dense(x, x, grid, cols, diag=True).double() - (W * W).sum(-1).double()).abs().max().item() <= 10 * tol


@pytest.mark.parametrize("name", CASES)
def test_grid_helpers_match_the_reference(name):
    grid, _, _ = _case(name)
    bounds = [tuple(b) for b in GOLD[f"{name}_bounds"].tolist()]
    mine = create_grid([g.numel() for g in grid], bounds, dtype=grid[0].dtype)
    for a, b in zip(mine, grid):
        assert torch.equal(a, b)
    h = (bounds[0][1] - bounds[0][0]) / (grid[0].numel() - 2)
    assert abs(float(mine[0][0]) - (bounds[0][0] - h)) < 1e-6 * max(1.0, abs(bounds[0][0]))       # extended by one spacing of (hi - lo) / (m - 2)
    assert torch.equal(create_data_from_grid(mine), torch.from_numpy(GOLD[f"{name}_data"]))


def test_choose_grid_size_and_scale_to_bounds():
    for n, d, ratio, want in GOLD["choose_grid_size"].tolist():
        assert choose_grid_size(torch.zeros(int(n), int(d)), ratio) == int(want) == int(ratio * math.pow(n, 1.0 / d))
    assert choose_grid_size(torch.zeros(50), 2.0, kronecker_structure=False) == 100.0
    s = ScaleToBounds(-1.0, 1.0)
    x = torch.linspace(3.0, 7.0, 9)
    out = s.train()(x)
    assert abs(float(out.min()) + 0.95) < 1e-6 and abs(float(out.max()) - 0.95) < 1e-6
    assert float(s.eval()(torch.tensor([100.0])).max()) <= 0.95 + 1e-6


def test_constructor_errors_and_buffers():
    with pytest.raises(RuntimeError, match="num_dims must be supplied"):
        GridInterpolationKernel(RBFKernel(), grid_size=8)
    with pytest.raises(RuntimeError, match="disagrees with the number of supplied"):
        GridInterpolationKernel(RBFKernel(), grid_size=8, num_dims=3, grid_bounds=[(0, 1), (0, 1)])
    with pytest.raises(RuntimeError, match="do not match num_dims"):
        GridInterpolationKernel(RBFKernel(), grid_size=[8, 8, 8], num_dims=2)
    with pytest.raises(ValueError, match="at least 4"):
        GridInterpolationKernel(RBFKernel(), grid_size=[8, 3], grid_bounds=[(0, 1), (0, 1)])
    k = GridInterpolationKernel(RBFKernel(), grid_size=[9, 6], grid_bounds=[(0, 1), (-1, 1)])
    assert set(dict(k.named_buffers())) >= {"grid_0", "grid_1", "has_initialized_grid"} and bool(k.has_initialized_grid)
    assert [g.numel() for g in k.grid] == [9, 6] and not k.grid_is_dynamic
    with pytest.raises(RuntimeError, match="same number of dimensions"):
        k.update_grid([k.grid[0]])
    with pytest.raises(RuntimeError, match="Received data that was out of bounds for the specified grid"):
        k(torch.tensor([[0.5, 1.9]]))
    k.update_grid(create_grid([9, 6], [(0, 1), (-2, 2)]))
    assert k(torch.tensor([[0.5, 1.9]])).shape == (1, 1)


def test_dynamic_grid():
    k = GridInterpolationKernel(RBFKernel(), grid_size=16, num_dims=2)
    assert k.grid_is_dynamic and not bool(k.has_initialized_grid)
    g = torch.Generator().manual_seed(3)
    x = 4.0 + torch.rand(30, 2, generator=g)
    k(x).to_dense()
    assert bool(k.has_initialized_grid)
    lo, hi = x.min(0)[0].tolist(), x.max(0)[0].tolist()
    for i in range(2):                                   # the 2.01-spacing rule of the reference's forward
        sp = (hi[i] - lo[i]) / (16 - 4.02)
        assert k.grid_bounds[i] == (lo[i] - 2.01 * sp, hi[i] + 2.01 * sp)
    first = [g_.clone() for g_ in k.grid]
    inside = x[:10] * 0.5 + x.mean(0) * 0.5
    k(inside).to_dense()                                 # inside the tight bounds: the grid is left alone
    assert all(torch.equal(a, b) for a, b in zip(first, k.grid))
    k(x + 3.0).to_dense()                                # outside: rebuilt
    assert not torch.equal(first[0], k.grid[0])


@pytest.mark.parametrize("batched", [False, True])
def test_reference_test_standard(batched):
    """The reference's test_grid_interpolation_kernel.py::test_standard on the dense path: grid 128^2, bounds +-1.2, five clamped normal points,
    default lengthscale; || K_ski - K_rbf ||_F < 2e-5 (the reference's bound)."""
    torch.manual_seed(0)
    base = RBFKernel(ard_num_dims=2)
    kernel = GridInterpolationKernel(base, num_dims=2, grid_size=128, grid_bounds=[(-1.2, 1.2)] * 2)
    x = torch.randn(3, 5, 2).clamp(-1, 1) if batched else torch.randn(5, 2).clamp(-1, 1)
    with gpytorch_amd.settings.use_toeplitz(True):
        K = gpytorch_amd.to_dense(kernel(x, x))
    with gpytorch_amd.settings.use_toeplitz(False):
        K2 = gpytorch_amd.to_dense(kernel(x, x))
    assert torch.equal(K, K2)
    z = x / base.lengthscale
    want = torch.exp(-0.5 * (z.unsqueeze(-2) - z.unsqueeze(-3)).pow(2).sum(-1))
    assert K.shape == want.shape
    assert (K - want).norm().item() < 2e-5
    assert (kernel(x, x, diag=True) - K.diagonal(dim1=-2, dim2=-1)).abs().max().item() < 1e-6


def _hyper_case(kind, ard, d):
    g = torch.Generator().manual_seed(17 + d)
    sizes = {1: (12,), 2: (9, 6), 3: (7, 6, 5)}[d]
    grid = create_grid(list(sizes), [(0.0, 1.0)] * d, dtype=torch.float64)
    x = torch.rand(20, d, generator=g, dtype=torch.float64)
    base = {"rbf": RBFKernel, "rq": RQKernel, "matern52": lambda **kw: MaternKernel(nu=2.5, **kw)}[kind](**({"ard_num_dims": d} if ard else {}))
    base = base.double()
    base.lengthscale = torch.tensor([0.3, 0.5, 0.7][:d]) if ard else 0.4
    if kind == "rq":
        base.alpha = 1.7
    return grid, x, base, g


@pytest.mark.parametrize("kind,ard,d,inner,outer", [("rbf", False, 1, False, False), ("rbf", True, 2, True, False), ("rbf", True, 3, False, True),
                                                    ("rq", False, 2, True, True), ("rq", True, 3, False, False), ("matern52", True, 2, False, True)])
def test_gradient_assembly(kind, ard, d, inner, outer):
    """sum_c a_c^T (kron T_i) b_c differentiated through the Toeplitz columns (``ski.bilinear`` + the base kernel's own columns) against autograd
    through ski_ref's dense K, in float64."""
    grid, x, base, g = _hyper_case(kind, ard, d)
    kern = ScaleKernel(base).double() if inner else base
    if inner:
        kern.outputscale = 1.3
    scale = torch.tensor([0.8], dtype=torch.float64, requires_grad=True) if outer else None
    t = 3
    left, right = torch.randn(20, t, generator=g, dtype=torch.float64), torch.randn(20, t, generator=g, dtype=torch.float64)
    params = [p for p in kern.parameters()]
    # the library's assembly: A = W^T left, B = W^T right, then the bilinear form on the grid
    W = ski.interp_dense_w(x, grid)
    cols = ski.toeplitz_columns(kern, grid)
    val, gcols = ski.bilinear((W.T @ left).T.contiguous(), (W.T @ right).T.contiguous(), cols)
    sc = 1.0 if scale is None else scale.detach().reshape(())
    mine = torch.autograd.grad(cols, params, [gc * sc for gc in gcols], allow_unused=True)
    # the oracle: autograd through the dense K of ski_ref
    ls = base.lengthscale
    rcols = R.columns(kind, grid, ls, kern.outputscale if inner else None, base.alpha if kind == "rq" else None)
    K = R.k_ski(x, x, grid, rcols, scale)
    obj = (left * (K @ right)).sum()
    want = torch.autograd.grad(obj, params + ([scale] if outer else []), allow_unused=True)
    assert abs(float(val * sc) - float(obj.detach())) <= 1e-10 * max(1.0, abs(float(obj.detach())))
    for a, b in zip(mine, want):
        assert (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item())
    if outer:
        assert abs(float(val) - float(want[-1])) <= 1e-10 * max(1.0, abs(float(want[-1])))
    # and ski_dense is the same matrix
    assert (ski.ski_dense(x, x, grid, cols) * sc - K).abs().max().item() <= 1e-12


class _Fake:
    """A tensor-like stand-in that claims to live on the device: ``ski_native`` is pure (shapes, dtypes, device type), so no GPU is needed."""

    def __init__(self, shape, dtype=torch.float32, device="cuda", requires_grad=False):
        self.shape, self.dtype, self.device, self.requires_grad = torch.Size(shape), dtype, torch.device(device), requires_grad

    def dim(self):
        return len(self.shape)


def test_ski_native_envelope():
    def kern(sizes, base=None):
        return GridInterpolationKernel(RBFKernel() if base is None else base, grid_size=list(sizes), grid_bounds=[(0.0, 1.0)] * len(sizes))

    k2 = kern((9, 6))
    assert ski_native(k2, _Fake((10, 2)))
    assert ski_native(k2, _Fake((10, 2)), _Fake((7, 2)))
    assert ski_native(kern((8,)), _Fake((10, 1))) and ski_native(kern((7, 6, 5)), _Fake((10, 3)))
    assert not ski_native(k2, _Fake((10, 2), dtype=torch.float64))
    assert not ski_native(k2, _Fake((10, 2)), _Fake((7, 2), dtype=torch.float64))
    assert not ski_native(k2, _Fake((3, 10, 2)))                                         # batch
    assert not ski_native(k2, _Fake((10, 2), device="cpu"))
    assert not ski_native(k2, _Fake((10, 2), requires_grad=True))                        # input gradients are not native
    assert not ski_native(k2, _Fake((10, 2)), last_dim_is_batch=True)
    assert not ski_native(kern((5, 5, 5, 5)), _Fake((10, 4)))                            # d > 3
    assert not ski_native(k2.double(), _Fake((10, 2)))                                   # float64 grid
    assert ski_native(kern((256, 256, 256)), _Fake((10, 3)))                             # M = 2^24: the limit itself
    assert not ski_native(kern((257, 256, 256)), _Fake((10, 3)))
    for base in (MaternKernel(nu=1.5), RQKernel(), ScaleKernel(RBFKernel()), ScaleKernel(ScaleKernel(MaternKernel(nu=0.5)))):
        assert ski_native(kern((9, 6), base), _Fake((10, 2)))
    assert not ski_native(kern((9, 6), RBFKernel() + MaternKernel()), _Fake((10, 2)))    # not one of the dense differentiable families
    assert not ski_native(kern((9, 6), RBFKernel(batch_shape=torch.Size([2]))), _Fake((10, 2)))
    small = kern((9, 6))
    small.update_grid([small.grid[0], small.grid[1][:3]])
    with pytest.raises(ValueError, match="at least 4"):
        ski_native(small, _Fake((10, 2)))
    with pytest.raises(ValueError, match="at least 4"):
        B.SkiGridSpec([torch.linspace(0, 1, 3)])


def test_abi_argument_validation_without_gpu():
    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5
    raw = ctypes.create_string_buffer(256)
    buf = ctypes.addressof(raw)          # (non-null host address: never dereferenced before the checks)
    dbl, ints = ctypes.c_double * 3, ctypes.c_int * 3
    g0, hh = dbl(0.0, 0.0, 0.0), dbl(0.1, 0.1, 0.1)

    def prep(d=2, m=(9, 6, 5), X=buf, keys=buf, ldx=2, n=10, g0_=g0, h_=hh):
        return h.gpamd_ski_prepare_f32(X, ldx, n, d, g0_, h_, ints(*m), keys, None)

    def interp(d=2, m=(9, 6, 5), X=buf, U=buf, Out=buf, ldg=54, ld=12, ldx=2, n=10, t=2):
        return h.gpamd_ski_interp_f32(X, ldx, n, d, g0, hh, ints(*m), None, U, ldg, t, Out, ld, None)

    def interp_t(d=2, m=(9, 6, 5), X=buf, perm=buf, cs=buf, V=buf, U=buf, ldv=12, ldg=54, nch=0, co=None, cb=None, ce=None, ws=None, nws=0, t=2):
        return h.gpamd_ski_interp_t_f32(X, 2, 10, d, g0, hh, ints(*m), perm, cs, co, cb, ce, nch, V, ldv, t, U, ldg, ws, nws, None)

    for call, what in ((prep, b"ski_prepare"), (interp, b"ski_interp"), (interp_t, b"ski_interp_t")):
        assert call(d=0) == -2 and call(d=4) == -2 and h.gpamd_last_error() == what + b": d must be in 1..3"
        assert call(m=(9, 3, 5)) == -1 and h.gpamd_last_error() == what + b": every grid axis needs at least 4 nodes"
        assert call(d=3, m=(257, 256, 256)) == -2 and h.gpamd_last_error() == what + b": the grid has more than 2^24 nodes"
        assert call(X=None) == -1 and h.gpamd_last_error().startswith(what + b": null pointer")
    assert prep(keys=None) == -1 and prep(ldx=1) == -1 and b"row stride" in h.gpamd_last_error()
    assert prep(g0_=None) == -1 and b"grid description" in h.gpamd_last_error()
    assert prep(h_=dbl(0.1, 0.0, 0.1)) == -1 and b"spacing must be positive" in h.gpamd_last_error()
    assert interp(U=None) == -1 and interp(Out=None) == -1
    assert interp(ldg=53) == -1 and h.gpamd_last_error().startswith(b"ski_interp: leading dimensions")
    assert interp(ld=9) == -1 and h.gpamd_last_error().startswith(b"ski_interp: leading dimensions")
    assert interp_t(perm=None) == -1 and interp_t(cs=None) == -1 and interp_t(V=None) == -1 and interp_t(U=None) == -1
    assert interp_t(ldv=9) == -1 and interp_t(ldg=53) == -1 and h.gpamd_last_error().startswith(b"ski_interp_t: leading dimensions")
    assert interp_t(nch=2) == -1 and b"chunk lists" in h.gpamd_last_error()
    need = h.gpamd_ski_workspace_floats(2, 2, 2)
    assert need == 2 * 16 * 2 and h.gpamd_ski_workspace_floats(3, 5, 11) == 5 * 64 * 11 and h.gpamd_ski_workspace_floats(4, 1, 1) == 0
    assert interp_t(nch=2, co=buf, cb=buf, ce=buf, ws=buf, nws=need - 1) == -3
    assert h.gpamd_last_error().startswith(b"ski_interp_t: workspace smaller")
    assert (B.SKI_P, B.SKI_G, B.SKI_C, B.SKI_LONG, B.SKI_MAX_DIM, B.SKI_MAX_NODES) == (256, 256, 4, 256, 3, 1 << 24)


@pytest.mark.parametrize("m", [B.TOEPLITZ_DENSE_MAX, B.TOEPLITZ_DENSE_MAX + 1, 1500])
def test_long_axes_multiply_through_the_fft(m):
    """Above ``TOEPLITZ_DENSE_MAX`` nodes an axis multiplies through the circulant embedding: the same product and the same column gradient as the
    dense matrix, in float64 to rounding."""
    g = torch.Generator().manual_seed(m)
    col = torch.exp(-0.5 * (torch.arange(m, dtype=torch.float64) / 25.0).pow(2)).requires_grad_(True)
    c2 = torch.rand(5, generator=g, dtype=torch.float64)
    u = torch.randn(3, 5 * m, generator=g, dtype=torch.float64)
    op = B.toeplitz_prepare(col)
    assert op[0] == ("dense" if m <= B.TOEPLITZ_DENSE_MAX else "fft")
    got = B.kron_matmul([op, B.toeplitz_prepare(c2)], u)
    want = R.kuu_matmul([col, c2], u.t()).t()
    assert (got - want).abs().max().item() <= 1e-11 * want.abs().max().item()
    ga, gb = torch.autograd.grad((got * u).sum(), col)[0], torch.autograd.grad((want * u).sum(), col)[0]
    assert (ga - gb).abs().max().item() <= 1e-11 * gb.abs().max().item()
