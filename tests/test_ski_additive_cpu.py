"""Additive KISS-GP (AdditiveStructureKernel over GridInterpolationKernel(num_dims=1)) without a GPU: the per-column interpolation against the
reference's own outputs under ``_compute_grid(last_dim_is_batch=True)`` (tests/golden/ski_additive_values.npz, made by executing the reference), the
dense branch against the float64 oracle ``tests/ski_additive_ref.py``, the pooled dynamic grid, how a lengthscale [1, k] reaches the axes (the
reference's executed broadcast), the native envelope, the argument checks of the four entry points and the grid-side product."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import gpytorch_amd as g
from gpytorch_amd import backend as B
from gpytorch_amd import ski
from gpytorch_amd.kernels import (AdditiveStructureKernel, GridInterpolationKernel, MaternKernel, PeriodicKernel, RBFKernel, RQKernel, ScaleKernel,
                                  ski_additive_native)
from gpytorch_amd.operators import DenseLinearOperator
from tests import ski_additive_ref as A
from tests import ski_ref as R
from tests.test_ski_cpu import _Fake

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ski_additive_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files if k.endswith("_val")})


def _additive(gk, d, outer=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AdditiveStructureKernel(ScaleKernel(gk) if outer else gk, num_dims=d)


def test_fixture_covers_the_cases():
    assert {GOLD[f"{c}_x"].shape[1] for c in CASES} == {2, 5}
    assert {GOLD[f"{c}_x"].dtype for c in CASES} == {np.dtype("float32"), np.dtype("float64")}
    assert all(GOLD[f"{c}_x"].shape[0] <= 40 for c in CASES)


@pytest.mark.parametrize("name", CASES)
def test_interpolation_matches_the_reference(name):
    """The [d, n, 4] index / value layout of the reference's dimension batch: column q of x on the ONE shared axis is ``ski.interp_axis``."""
    axis, x = torch.from_numpy(GOLD[f"{name}_grid"]), torch.from_numpy(GOLD[f"{name}_x"])
    idx, val = torch.from_numpy(GOLD[f"{name}_idx"]), torch.from_numpy(GOLD[f"{name}_val"])
    n, d = x.shape
    assert idx.shape == (d, n, 4) and val.shape == (d, n, 4)
    tol = 1e-12 if x.dtype == torch.float64 else 1e-6      # (float32 cases: the reference's own float32 index arithmetic is what is allowed for)
    spec = B.SkiGridSpec([axis])
    m = axis.numel()
    edge_any = False
    for q in range(d):
        Wref = torch.zeros(n, m, dtype=val.dtype).scatter_add_(1, idx[q], val[q])
        b, w, edge = ski.interp_axis(x[:, q], spec.g0[0], spec.h[0], m)
        W = torch.zeros(n, m, dtype=x.dtype).scatter_add_(1, b.unsqueeze(-1) + torch.arange(4), w)
        assert (W.double() - Wref.double()).abs().max().item() <= tol
        edge_any |= bool(edge.any())
    assert edge_any and (val < 0).any()
    Wadd = ski.interp_dense_w(x, [axis] * d, additive=True)
    Wgold = torch.cat([torch.zeros(n, m, dtype=val.dtype).scatter_add_(1, idx[q], val[q]) for q in range(d)], dim=1)
    assert Wadd.shape == (n, d * m) and (Wadd.double() - Wgold.double()).abs().max().item() <= tol
    assert (A.dense_w_add(x, [axis] * d) - Wgold.double()).abs().max().item() <= tol


def _problem(d, m=12, n=30, k=None, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x1 = torch.rand(n, d, generator=gen, dtype=torch.float64)
    x2 = torch.rand(n - 9, d, generator=gen, dtype=torch.float64)
    ls = 0.25 + 0.5 * torch.rand(1 if k is None else k, generator=gen, dtype=torch.float64)
    return x1, x2, ls


@pytest.mark.parametrize("d,ard", [(2, False), (2, True), (5, True)])
def test_dense_branch_against_the_oracle(d, ard):
    """``ski_dense(additive=True)``, its ``diag`` and ``GridInterpolationKernel(..., last_dim_is_batch=True)`` in float64 at 1e-12."""
    x1, x2, ls = _problem(d, k=d if ard else None)
    gk = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=d if ard else None)), grid_size=12, num_dims=1, grid_bounds=[(0.0, 1.0)]).double()
    gk.base_kernel.base_kernel.lengthscale = ls
    gk.base_kernel.outputscale = torch.tensor(1.3, dtype=torch.float64)
    axis = gk.grid[0]
    grid = [axis] * d
    cols = R.columns("rbf", grid if ard else grid[:1], ls, torch.tensor(1.3, dtype=torch.float64))
    want, sq = A.k_ski_add(x1, x2, grid, cols), A.k_ski_add(x1, x1, grid, cols)
    assert (ski.ski_dense(x1, x2, grid, cols, additive=True) - want).abs().max().item() <= 1e-12
    assert (ski.ski_dense(x1, x1, grid, cols, diag=True, additive=True) - sq.diagonal()).abs().max().item() <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = gk(x1, x2, last_dim_is_batch=True)
        bdiag = gk(x1, diag=True, last_dim_is_batch=True)
    assert torch.is_tensor(batch) and batch.shape == (d, 30, 21) and bdiag.shape == (d, 30)
    assert (batch.sum(0) - want).abs().max().item() <= 1e-12 and (bdiag.sum(0) - sq.diagonal()).abs().max().item() <= 1e-12
    for q in range(d):                                       # member q is the one-dimensional interpolated kernel of column q
        one = R.k_ski(x1[:, q: q + 1], x2[:, q: q + 1], [axis], [cols[q if ard else 0]])
        assert (batch[q] - one).abs().max().item() <= 1e-12
    ak = _additive(gk, d).double()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        op = ak(x1, x2)
        assert isinstance(op, DenseLinearOperator) and (op.to_dense() - want).abs().max().item() <= 1e-12
        assert (ak(x1, diag=True) - sq.diagonal()).abs().max().item() <= 1e-12


def test_num_dims_other_than_one_is_refused():
    gk = GridInterpolationKernel(RBFKernel(), grid_size=8, num_dims=2, grid_bounds=[(0.0, 1.0)] * 2)
    with warnings.catch_warnings(), pytest.raises(AssertionError, match="num_dims == 1"):
        warnings.simplefilter("ignore")
        gk(torch.rand(5, 2), last_dim_is_batch=True)
    gk1 = GridInterpolationKernel(RBFKernel(ard_num_dims=3), grid_size=8, num_dims=1, grid_bounds=[(0.0, 1.0)])
    with warnings.catch_warnings(), pytest.raises(RuntimeError, match="do not broadcast"):      # 3 lengthscales against 2 dimensions
        warnings.simplefilter("ignore")
        gk1(torch.rand(5, 2), last_dim_is_batch=True)


def test_dynamic_grid_pools_all_columns():
    """``x.reshape(-1, self.num_dims)`` (grid_interpolation_kernel.py:150-181): the ONE axis is fitted to the minimum and maximum over ALL columns,
    and a coordinate outside a fixed grid is the reference's out-of-bounds error whatever its column."""
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(30, 3, generator=gen) * torch.tensor([1.0, 4.0, 0.5]) + torch.tensor([0.0, 2.0, -1.0])
    gk = GridInterpolationKernel(RBFKernel(), grid_size=16, num_dims=1)
    ak = _additive(gk, 3)
    ak(x).to_dense()
    assert bool(gk.has_initialized_grid)
    lo, hi = float(x.min()), float(x.max())
    sp = (hi - lo) / (16 - 4.02)
    assert gk.grid_bounds == ((lo - 2.01 * sp, hi + 2.01 * sp),)
    first = gk.grid[0].clone()
    ak(x[:10] * 0.5 + x.mean() * 0.5).to_dense()            # inside the tight bounds: the grid is left alone
    assert torch.equal(first, gk.grid[0])
    fixed = _additive(GridInterpolationKernel(RBFKernel(), grid_size=16, num_dims=1, grid_bounds=[(0.0, 1.0)]), 3)
    bad = torch.rand(10, 3, generator=gen)
    bad[4, 2] = 1.5                                          # one coordinate, in the LAST column
    with pytest.raises(RuntimeError, match="out of bounds"):
        fixed(bad).to_dense()
    with pytest.raises(RuntimeError, match="out of bounds"):
        fixed(torch.rand(10, 3, generator=gen), bad).to_dense()


@pytest.mark.parametrize("kind", ["rbf", "matern", "rq"])
@pytest.mark.parametrize("k", [1, 3])
def test_lengthscales_reach_the_axes_as_in_the_reference(kind, k):
    """How a lengthscale [1, k] reaches the d axes.  The reference evaluates the base kernel on the ONE-column grid under ``last_dim_is_batch``
    (grid_kernel.py:142-146): ``x.div(lengthscale)`` broadcasts the column into k scaled copies (rbf_kernel.py:77-78), and ``covar_dist`` THEN turns
    the last dimension into a batch (kernel.py:336-338) -- k Toeplitz columns, member j at lengthscale l_j, NOT one column at
    (sum_j l_j^-2)^(-1/2).  k = d puts l_q on input column q; k = 1 is repeated.  Checked against (a) the reference's executed output in the
    fixture and (b) a float64 restatement of that broadcast."""
    axis = torch.from_numpy(GOLD["col_axis"])
    ls = torch.from_numpy(GOLD[f"col_ls_k{k}"])
    gold = torch.from_numpy(GOLD[f"col_{kind}_k{k}"])
    assert gold.shape == (k, axis.numel())
    base = {"rbf": RBFKernel, "matern": lambda **kw: MaternKernel(nu=2.5, **kw), "rq": RQKernel}[kind](ard_num_dims=k if k > 1 else None).double()
    base.lengthscale = ls
    if kind == "rq":
        base.alpha = torch.tensor(float(GOLD["col_alpha"]), dtype=torch.float64)
    d = 3
    cols = ski.additive_columns(base, axis, d)
    assert len(cols) == (1 if k == 1 else d)                 # a single lengthscale: ONE column shared by every axis
    # (b) the broadcast restated: [m, 1] / [1, k] -> [m, k] -> transpose -> k members of one column each
    scaled = (axis.unsqueeze(-1) / ls.reshape(1, k)).transpose(-1, -2).unsqueeze(-1)            # [k, m, 1]
    dist2 = (scaled - scaled[:, :1]).pow(2).sum(-1)                                             # [k, m]
    if kind == "rbf":
        restated = torch.exp(-0.5 * dist2)
    elif kind == "rq":
        a = float(GOLD["col_alpha"])
        restated = (1.0 + dist2 / (2.0 * a)).pow(-a)
    else:
        r = dist2.sqrt()
        restated = (1.0 + 5.0 ** 0.5 * r + 5.0 / 3.0 * r * r) * torch.exp(-(5.0 ** 0.5) * r)
    assert (restated - gold).abs().max().item() <= 1e-12
    for q, c in enumerate(cols):
        assert (c.detach() - gold[q if k > 1 else 0]).abs().max().item() <= 1e-12
    if k > 1:                                                # ... and it is NOT the effective-lengthscale column
        eff = float(ls.pow(-2).sum().pow(-0.5))
        assert (torch.exp(-0.5 * ((axis - axis[0]) / eff).pow(2)) - cols[0].detach()).abs().max().item() > 0.05 or kind != "rbf"
    # autograd splits over the l_j: member j's column depends on l_j alone
    if k > 1:
        gr = torch.autograd.grad(cols[1].sum(), base.raw_lengthscale)[0].reshape(-1)
        assert gr[1] != 0 and gr[0] == 0 and gr[2] == 0


def test_ski_additive_native_truth_table():
    def kern(d=3, m=9, base=None, inner=False, outer=True, num_dims=None, grid_kernel=None):
        base = RBFKernel() if base is None else base
        gk = GridInterpolationKernel(ScaleKernel(base) if inner else base, grid_size=m, num_dims=1, grid_bounds=[(0.0, 1.0)]) if grid_kernel is None \
            else grid_kernel
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return AdditiveStructureKernel(ScaleKernel(gk) if outer else gk, num_dims=d if num_dims is None else num_dims)

    x = _Fake((10, 3))
    assert ski_additive_native(kern(), x) and ski_additive_native(kern(outer=False), x) and ski_additive_native(kern(inner=True), x, _Fake((7, 3)))
    # the base: a GridInterpolationKernel with num_dims == 1, bare or inside ONE unbatched ScaleKernel
    assert not ski_additive_native(kern(grid_kernel=RBFKernel()), x)
    assert not ski_additive_native(kern(grid_kernel=GridInterpolationKernel(RBFKernel(), grid_size=9, grid_bounds=[(0.0, 1.0)] * 3)), x)
    assert not ski_additive_native(kern(grid_kernel=ScaleKernel(GridInterpolationKernel(RBFKernel(), grid_size=9, num_dims=1, grid_bounds=[(0.0, 1.0)]))), x)
    batched = kern()
    batched.base_kernel = ScaleKernel(batched.base_kernel.base_kernel, batch_shape=torch.Size([2]))
    assert not ski_additive_native(batched, x)
    # columns_native of the grid kernel's base kernel
    for base in (MaternKernel(nu=1.5), RQKernel(), ScaleKernel(MaternKernel(nu=0.5)), PeriodicKernel(), RBFKernel(ard_num_dims=3)):
        assert ski_additive_native(kern(base=base), x)
    assert not ski_additive_native(kern(base=RBFKernel() + MaternKernel()), x)
    assert not ski_additive_native(kern(base=RBFKernel(batch_shape=torch.Size([2]))), x)
    assert not ski_additive_native(kern(base=RBFKernel(ard_num_dims=2)), x)              # 2 lengthscales against 3 dimensions
    assert not ski_additive_native(kern(base=PeriodicKernel(ard_num_dims=3)), x)         # Periodic with several lengthscales: the dense branch
    # the inputs: float32, on the device, no requires_grad, no batch shape
    assert not ski_additive_native(kern(), _Fake((10, 3), dtype=torch.float64))
    assert not ski_additive_native(kern(), x, _Fake((7, 3), dtype=torch.float64))
    assert not ski_additive_native(kern(), _Fake((10, 3), device="cpu"))
    assert not ski_additive_native(kern(), _Fake((10, 3), requires_grad=True))
    assert not ski_additive_native(kern(), _Fake((2, 10, 3)))
    assert not ski_additive_native(kern().double(), x)                                   # float64 grid
    assert not ski_additive_native(kern(), x, last_dim_is_batch=True)
    # 2 <= d <= 16 and d == num_dims
    assert ski_additive_native(kern(d=2), _Fake((10, 2))) and ski_additive_native(kern(d=16), _Fake((10, 16)))
    assert not ski_additive_native(kern(d=1), _Fake((10, 1))) and not ski_additive_native(kern(d=17), _Fake((10, 17)))
    assert not ski_additive_native(kern(num_dims=4), x)
    # m >= 4 (the constructor refuses fewer), at most 2^24 nodes in all
    assert ski_additive_native(kern(m=4), x)
    with pytest.raises(ValueError, match="at least 4"):
        kern(m=3)
    assert ski_additive_native(kern(d=16, m=1 << 20), _Fake((10, 16))) and not ski_additive_native(kern(d=16, m=(1 << 20) + 1), _Fake((10, 16)))


def _reference_data(n):
    t = torch.arange(n, dtype=torch.float64) / (n - 1)
    X = torch.stack([t.repeat_interleave(n), t.repeat(n)], dim=-1)
    return X, torch.sin(X[:, 0]) + torch.cos(X[:, 1])


def test_cpu_float64_model_equals_the_oracle():
    """The reference test's model and data, shrunk to 8 x 8 training points and m = 12, on the CPU in float64: the dense branch; the marginal log
    likelihood and the posterior equal the oracle's by dense Cholesky."""
    gen = torch.Generator().manual_seed(1)
    X, y = _reference_data(8)
    y = y + torch.randn(64, generator=gen, dtype=torch.float64) / 20.0
    Xs, _ = _reference_data(5)

    class GPRegressionModel(g.models.ExactGP):
        def __init__(self, train_x, train_y, likelihood):
            super().__init__(train_x, train_y, likelihood)
            self.mean_module = g.means.ZeroMean()
            self.base_covar_module = ScaleKernel(RBFKernel(ard_num_dims=2))
            self.covar_module = _additive(GridInterpolationKernel(self.base_covar_module, grid_size=12, num_dims=1), 2)

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.GaussianLikelihood().double()
    model = GPRegressionModel(X, y, lik).double()
    ls, os_, noise = torch.tensor([0.3, 0.6], dtype=torch.float64), torch.tensor(0.8, dtype=torch.float64), torch.tensor(0.05, dtype=torch.float64)
    model.base_covar_module.base_kernel.lengthscale, model.base_covar_module.outputscale, lik.noise = ls, os_, noise
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.train()
        lik.train()
        assert isinstance(model.covar_module(X), DenseLinearOperator)
        val = g.ExactMarginalLogLikelihood(lik, model)(model(X), y)
        axis = model.covar_module.base_kernel.grid[0]
        grid = [axis] * 2
        cols = R.columns("rbf", grid, ls, os_)
        assert abs(float(val) - float(A.mll(X, y, grid, cols, None, noise))) <= 1e-9
        model.eval()
        lik.eval()
        with torch.no_grad():
            pred = model(Xs)
        assert torch.equal(axis, model.covar_module.base_kernel.grid[0])         # (the test lattice lies inside the training lattice: same grid)
        mu, cov = A.posterior(X, y, Xs, grid, cols, None, noise)
        assert (pred.mean - mu).abs().max().item() <= 1e-8
        assert (pred.covariance_matrix - cov).abs().max().item() <= 1e-8


def test_abi_symbols_and_argument_validation_without_gpu():
    from gpytorch_amd import _lib

    h = _lib.lib()
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = {"gpamd_ski_add_prepare_f32": (i, [p, i64, i, i, p, p, p, p, p]),
            "gpamd_ski_add_interp_f32": (i, [p, i64, i, i, p, p, p, p, p, i64, i, p, i64, p]),
            "gpamd_ski_add_workspace_floats": (i64, [i, i, i]),
            "gpamd_ski_add_interp_t_f32": (i, [p, i64, i, i, p, p, p, p, p, p, p, p, i, p, i64, i, p, i64, p, i64, p])}
    for name, (res, args) in want.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    raw = ctypes.create_string_buffer(256)
    buf = ctypes.addressof(raw)          # (non-null host address: never dereferenced before the checks)

    def arrays(d, m):
        return (ctypes.c_double * d)(*[0.0] * d), (ctypes.c_double * d)(*[0.1] * d), (ctypes.c_int * d)(*m)

    def prep(d=2, m=(9, 6), X=buf, keys=buf, ldx=2):
        return h.gpamd_ski_add_prepare_f32(X, ldx, 10, d, *arrays(d, m), keys, None)

    def interp(d=2, m=(9, 6), X=buf, U=buf, Out=buf, ldg=15, ld=12):
        return h.gpamd_ski_add_interp_f32(X, 2 if d == 2 else d, 10, d, *arrays(d, m), None, U, ldg, 2, Out, ld, None)

    def interp_t(d=2, m=(9, 6), X=buf, perm=buf, cs=buf, V=buf, U=buf, ldv=12, ldg=15, nch=0, co=None, cb=None, ce=None, ws=None, nws=0):
        return h.gpamd_ski_add_interp_t_f32(X, 2 if d == 2 else d, 10, d, *arrays(d, m), perm, cs, co, cb, ce, nch, V, ldv, 2, U, ldg, ws, nws, None)

    for call, what in ((prep, b"ski_add_prepare"), (interp, b"ski_add_interp"), (interp_t, b"ski_add_interp_t")):
        assert call(d=1, m=(9,)) == -2 and h.gpamd_last_error() == what + b": d must be in 2..16"
        assert call(d=17, m=(9,) * 17) == -2 and h.gpamd_last_error() == what + b": d must be in 2..16"
        assert call(m=(9, 3)) == -1 and h.gpamd_last_error() == what + b": every grid axis needs at least 4 nodes"
        assert call(d=3, m=(1 << 23, 1 << 23, 4)) == -2 and h.gpamd_last_error() == what + b": the grid has more than 2^24 nodes"
        assert call(X=None) == -1 and h.gpamd_last_error().startswith(what + b": null pointer")
    assert prep(keys=None) == -1 and prep(ldx=1) == -1 and b"row stride" in h.gpamd_last_error()
    assert interp(ldg=14) == -1 and interp(ld=9) == -1 and h.gpamd_last_error().startswith(b"ski_add_interp: leading dimensions")
    assert interp_t(perm=None) == -1 and interp_t(cs=None) == -1 and interp_t(ldv=9) == -1 and interp_t(ldg=14) == -1
    assert interp_t(nch=2) == -1 and b"chunk lists" in h.gpamd_last_error()
    need = h.gpamd_ski_add_workspace_floats(2, 3, 5)
    assert need == 3 * 4 * 5 and h.gpamd_ski_add_workspace_floats(1, 1, 1) == 0 and h.gpamd_ski_add_workspace_floats(17, 1, 1) == 0
    assert interp_t(nch=3, co=buf, cb=buf, ce=buf, ws=buf, nws=3 * 4 * 2 - 1) == -3 and h.gpamd_last_error().startswith(b"ski_add_interp_t: workspace smaller")
    assert (B.SKI_ADD_MIN_DIM, B.SKI_ADD_MAX_DIM) == (2, 16)


@pytest.mark.parametrize("m", [8, 1025])
@pytest.mark.parametrize("shared", [True, False])
def test_grid_matmul_additive(m, shared):
    """The block-diagonal grid-side product against the oracle over the dense (m = 8) and the FFT (m = 1025) Toeplitz branch, with ONE shared
    column ([m, d t] product) and with one column per axis; unequal axes; and the Kronecker structure still goes through ``kron_matmul``."""
    gen = torch.Generator().manual_seed(m)
    d, t = 3, 5
    axis = torch.linspace(0.0, 1.0, m, dtype=torch.float64)
    spec = B.SkiGridSpec([axis] * d, additive=True)
    assert spec.nodes == d * m and spec.cells == d * (m - 3) and spec.off == [0, m, 2 * m, 3 * m] and spec.key != B.SkiGridSpec([axis] * d).key
    cols = R.columns("rbf", [axis] * (1 if shared else d), torch.tensor([0.2] if shared else [0.1, 0.2, 0.4], dtype=torch.float64))
    U = torch.randn(t, spec.nodes, generator=gen, dtype=torch.float64)
    ops = [B.toeplitz_prepare(c) for c in cols]
    assert ops[0][0] == ("dense" if m <= B.TOEPLITZ_DENSE_MAX else "fft")
    got = B.grid_matmul(spec, ops, U)
    want = A.kuu_add_matmul(cols, spec.m, U.t()).t()
    assert got.shape == (t, spec.nodes) and (got - want).abs().max().item() <= 1e-10 * want.abs().max().item()
    assert (A.k_uu_add(cols, d) @ U.t() - want.t()).abs().max().item() <= 1e-10 * want.abs().max().item() if m == 8 else True
    # the gradient assembly through the shared / per-axis columns (``ski.bilinear``)
    At = torch.randn(t, spec.nodes, generator=gen, dtype=torch.float64)
    val, grads = ski.bilinear(At, U, cols, spec)
    cref = [c.clone().requires_grad_(True) for c in cols]
    ref = (At.t() * A.kuu_add_matmul(cref, spec.m, U.t())).sum()
    gref = torch.autograd.grad(ref, cref)
    assert abs(float(val) - float(ref)) <= 1e-10 * abs(float(ref)) and len(grads) == len(cols)
    assert all((a - b).abs().max().item() <= 1e-9 * b.abs().max().item() for a, b in zip(grads, gref))
    if m == 8:
        axes = [axis, torch.linspace(0.0, 1.0, 5, dtype=torch.float64)]
        sp2 = B.SkiGridSpec(axes, additive=True)
        c2 = R.columns("rbf", axes, torch.tensor([0.3], dtype=torch.float64))
        U2 = torch.randn(2, sp2.nodes, generator=gen, dtype=torch.float64)
        assert (B.grid_matmul(sp2, [B.toeplitz_prepare(c) for c in c2], U2).t() - A.kuu_add_matmul(c2, sp2.m, U2.t())).abs().max().item() <= 1e-12
        kron = B.SkiGridSpec(axes)
        U3 = torch.randn(2, kron.nodes, generator=gen, dtype=torch.float64)
        assert torch.equal(B.grid_matmul(kron, [B.toeplitz_prepare(c) for c in c2], U3), B.kron_matmul([B.toeplitz_prepare(c) for c in c2], U3))
