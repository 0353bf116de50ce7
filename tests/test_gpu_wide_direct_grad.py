"""The fused bilinear derivative of the wide clouds by direct differences (csrc/kv_wide_direct_grad.hpp, backend.kv_grad_wide_direct): clouds beyond the
norm rule of the Gram form, and Matern 1/2.  Ground truth: float64 on the CPU from the very float32 prepared rows the device holds, with the point-wise
formulas of tests/pointwise_ref.py (test_gpu_wide_grad._reference, which asserts that none of its sums cancels: |sum| >= 0.05 sum |terms| -- dk/ds < 0
for all four families and W is positive on average).  1e-3 relative per output is the project's bound for derivative kernels at high dimension
(tests/test_gpu_wide_grad.py, tests/test_gpu_highdim.py)."""
import ctypes as C
import math
import warnings

import pytest
import torch

from oracle import kernels as OK
from tests.test_gpu_wide_direct import _data
from tests.test_gpu_wide_grad import _reference, _vectors
from tests.util import rel_err

pytestmark = pytest.mark.gpu
BOUND = 1e-3


def _check(kind, p1, p2, lt, rt, mode, dev):
    from gpytorch_amd import backend as B

    assert B.wide_direct_f32(p1, p2) and not B.wide_f32(p1, p2)
    d = p1.d
    g_ref, gz_ref = _reference(kind, p1, p2, lt, rt)
    g, gz = B.kv_grad_wide_direct(p1, p2, lt.to(dev), rt.to(dev), iso=mode == "iso", want_gz1=mode == "gz")
    g = g.double().cpu()
    print(kind, d, mode, "g0", float(g[0]), float(g_ref[0]))
    assert abs(float(g[0] - g_ref[0])) < BOUND * abs(float(g_ref[0]))
    if mode == "iso":
        print("iso", float(g[1]), float(g_ref[1:].sum()))
        assert gz is None and abs(float(g[1] - g_ref[1:].sum())) < BOUND * abs(float(g_ref[1:].sum()))
        assert bool((g[2:] == 0).all())
    else:
        err = ((g[1 : 1 + d] - g_ref[1:]).abs() / g_ref[1:].abs()).max()
        print("per-dimension", float(err))
        assert float(err) < BOUND and bool((g[1 + d :] == 0).all())
    if mode == "gz":
        print("gz1", rel_err(gz, gz_ref))
        assert gz.shape == gz_ref.shape and rel_err(gz, gz_ref) < BOUND


# d: a chunk with one live dimension, whole chunks, one past a 128-dimension block, the maximum; ragged tiles on both sides, symmetric products (Matern 1/2:
# the S = 0 diagonal); (640, 2048): several slabs; t = 70: two passes of the W contraction
@pytest.mark.parametrize("kind,d,n,m,t,mode", [
    ("rbf", 33, 77, 131, 1, "iso"), ("matern12", 48, 333, 517, 11, "ard"), ("matern52", 129, 300, None, 33, "gz"), ("rbf", 512, 333, 517, 65, "ard"),
    ("matern12", 512, 300, None, 11, "gz"), ("matern32", 33, 333, 517, 65, "gz"), ("matern12", 129, 77, 131, 70, "iso"), ("matern52", 48, 300, None, 1, "iso"),
    ("matern32", 33, 640, 2048, 6, "gz"), ("rbf", 512, 77, 131, 33, "iso"), ("matern32", 129, 333, 517, 70, "ard"), ("matern12", 48, 300, None, 33, "gz"),
    ("matern52", 48, 640, 2048, 11, "ard")])
def test_sums_and_input_gradients(kind, d, n, m, t, mode, dev):
    p1, p2, _, _ = _data(kind, d, n, m, 1, dev, ard=mode != "iso")
    lt, rt = _vectors(n, m, t, torch.Generator().manual_seed(1), m is None)
    _check(kind, p1, p2, lt, rt, mode, dev)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("d,mode", [(33, "gz"), (512, "ard"), (512, "gz"), (33, "ard")])
def test_far_from_the_origin(kind, d, mode, dev):
    """_data's cloud with the common origin 300 lengthscales away: |z|^2 >= 5e4 in prepared coordinates for every point.  The reference depends on the
    differences of the prepared rows only; an implementation that expands the square in float32 (z_i^2 rs_i - 2 z_i u_i + v_i) loses every digit."""
    from gpytorch_amd import backend as B

    n, m, t = 300, 411, 11
    g0 = torch.Generator().manual_seed(0)
    X1, X2 = torch.rand(n, d, generator=g0), torch.rand(m, d, generator=g0)
    ls = math.sqrt(d) / 4 * (0.8 + 0.4 * torch.rand(d, generator=g0))
    shift = (X1.mean(0) - 300.0 * ls / math.sqrt(d)).to(dev)
    p1, p2 = B.prep_points(kind, X1.to(dev), ls.to(dev), shift), B.prep_points(kind, X2.to(dev), ls.to(dev), shift)
    assert float((p1.xp.double() ** 2).sum(1).min()) >= 5e4
    lt, rt = _vectors(n, m, t, g0, False)
    _check(kind, p1, p2, lt, rt, mode, dev)


def test_bitwise_reproducible(dev):
    from gpytorch_amd import backend as B

    p1, p2, _, _ = _data("matern52", 129, 333, 517, 1, dev, ard=True)
    lt, rt = (v.to(dev) for v in _vectors(333, 517, 33, torch.Generator().manual_seed(1), False))
    ga, za = B.kv_grad_wide_direct(p1, p2, lt, rt, want_gz1=True)
    gb, zb = B.kv_grad_wide_direct(p1, p2, lt, rt, want_gz1=True)
    assert torch.equal(ga, gb) and torch.equal(za, zb)


def test_routing_hyper_grads_with_input_gradients(dev):
    """Matern 1/2 at d = 40 with want_x1 / want_x2 (refused before this kernel) against float64 autograd through the dense kernel; with WIDE_KV = False
    the lengthscale and outputscale gradients come from the row-block path and agree."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    kind, n, m, d, t = "matern12", 300, 411, 40, 7
    g0 = torch.Generator().manual_seed(5)
    X1, X2 = torch.rand(n, d, generator=g0).double(), torch.rand(m, d, generator=g0).double()
    lt, rt = _vectors(n, m, t, g0, False)
    ls = (math.sqrt(d) / 4 * (0.8 + 0.4 * torch.rand(1, d, generator=g0))).double().requires_grad_(True)
    os_ = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    x1, x2 = X1.clone().requires_grad_(True), X2.clone().requires_grad_(True)
    K = OK.kernel_matrix(kind, x1, x2, ls, os_, x1_eq_x2=False, direct=True)
    ref = torch.autograd.grad((lt.double().t() * (K @ rt.double().t())).sum(), [ls, os_, x1, x2])
    lsd, osd, shift = ls.detach().float().to(dev), os_.detach().float().to(dev).reshape(1), X1.mean(0).float().to(dev)
    p1, p2 = B.prep_points(kind, X1.float().to(dev), lsd, shift), B.prep_points(kind, X2.float().to(dev), lsd, shift)
    assert B.wide_direct_f32(p1, p2)
    out = hyper_grads(p1, p2, lsd, osd, lt.to(dev), rt.to(dev), want_x1=True, want_x2=True)
    for got, want in zip(out, ref):
        print(rel_err(got.reshape(want.shape), want))
        assert rel_err(got.reshape(want.shape), want) < BOUND
    B.WIDE_KV = False
    try:
        slow = hyper_grads(p1, p2, lsd, osd, lt.to(dev), rt.to(dev))
    finally:
        B.WIDE_KV = True
    assert rel_err(slow[0], out[0]) < BOUND and rel_err(slow[1], out[1]) < BOUND


@pytest.mark.parametrize("kind,ard", [("rbf", True), ("matern12", False)])
def test_mll_backward_runs_fused_and_agrees_with_the_row_block_path(kind, ard, dev):
    """ExactMarginalLogLikelihood forward + backward at n = 2000 on a z-scored cloud of d = 64 (four latent factors, so that neighbours exist) at the
    default lengthscale, BBMM path with shared probes: no warning on the fused run, finite gradients, the lengthscale gradient within 2e-3
    (test_gpu_wide_grad.test_mll_backward_agrees_with_the_row_block_path's figure) of the WIDE_KV = False run."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from tests.test_gpu_generic import _model

    n, d = 2000, 64
    g0 = torch.Generator().manual_seed(0)
    F = torch.randn(n, 4, generator=g0, dtype=torch.float64)
    X = F @ torch.randn(4, d, generator=g0, dtype=torch.float64) + 0.05 * torch.randn(n, d, generator=g0, dtype=torch.float64)
    X = (X - X.mean(0)) / X.std(0)
    y = torch.sin(F[:, 0]) + 0.1 * torch.randn(n, generator=g0, dtype=torch.float64)
    Z = torch.randn(n, 10, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    grads = []
    for wide in (True, False):
        _, m, lik = _model(kind, X, y, math.log(2.0), 1.4, 0.1, dev, torch.float32, ard=ard)
        mll = g.ExactMarginalLogLikelihood(lik, m)
        m.train(), lik.train()
        B.WIDE_KV = wide
        try:
            with g.settings.max_cholesky_size(0), g.settings.deterministic_probes(True), warnings.catch_warnings():
                if wide:
                    warnings.simplefilter("error", RuntimeWarning)
                g.settings.deterministic_probes.probe_vectors = Z
                try:
                    mll(m(m.train_inputs[0]), m.train_targets).backward()
                finally:
                    g.settings.deterministic_probes.probe_vectors = None
        finally:
            B.WIDE_KV = True
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        grads.append(m.covar_module.base_kernel.raw_lengthscale.grad.clone())
    print(grads[0].abs().max(), rel_err(grads[0], grads[1]))
    assert float(grads[1].abs().max()) > 0 and rel_err(grads[0], grads[1]) < 2e-3


@pytest.mark.parametrize("d,short,code", [(32, 0, -2), (40, 1, -3)])
def test_argument_errors(d, short, code, dev):
    """d below the envelope (GPAMD_EUNSUPPORTED) and a workspace one double short (GPAMD_EWORKSPACE): the error code, and nothing written."""
    from gpytorch_amd import backend as B

    L, n, t = B.lib(), 200, 3
    p, _, _, _ = _data("rbf", 40, n, None, 1, dev)
    lt = torch.ones(t, n, device=dev)
    nd = int(L.gpamd_kv_wide_direct_grad_workspace_doubles(n, n, 40, t, 3))
    ws = torch.full((nd,), 7.0, device=dev, dtype=torch.float64)
    out = torch.full((2 + p.dp,), 7.0, device=dev)
    gz = torch.full((n, 40), 7.0, device=dev)
    ptr = lambda v: C.c_void_p(v.data_ptr())
    rc = L.gpamd_kv_wide_direct_grad_f32(B.kind_id(p), ptr(p.xp), n, ptr(p.xp), n, d, p.dp, ptr(lt), n, ptr(lt), n, t, 3, ptr(out), ptr(gz), 40, ptr(ws),
                                         nd - short, None)
    torch.cuda.synchronize()
    assert rc == code and bool((out == 7.0).all()) and bool((gz == 7.0).all()) and bool((ws == 7.0).all())
