"""GPU parity of the fused wide bilinear derivative (csrc/kv_wide_grad.hpp): float32 clouds of 33 .. 512 dimensions, RBF and Matern 3/2, 5/2.

Ground truth: float64 on the CPU from the very float32 prepared rows the device sees, with the point-wise formulas of ``tests/pointwise_ref.py``:
W = L^T R, g[0] = sum W k, g[1 + q] = sum W dk/ds (z_iq - z_jq)^2, Gz1[i] = 2 (z_i sum_j A_ij - sum_j A_ij z_j).  1e-3 relative per output is the
bound the derivative kernels are held to at high dimension (tests/test_gpu_highdim.py); the vector blocks are positive on average, so no sum cancels
(asserted on the reference: |sum| >= 0.05 sum |terms|)."""
import ctypes as C
import math

import pytest
import torch

from oracle import kernels as OK
from tests import pointwise_ref as PR
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu
BOUND = 1e-3


def _clouds(kind, d, n, m, dev, ard, seed=0):
    """The clouds of test_gpu_wide.py: U[0, 1]^d shifted by the mean of x1, lengthscale sqrt(d) / 4 (max |z|^2 <= ~4.5 for every d)."""
    from gpytorch_amd import backend as B

    g0 = torch.Generator().manual_seed(seed)
    X1 = torch.rand(n, d, generator=g0)
    X2 = X1 if m is None else torch.rand(m, d, generator=g0)
    ls = torch.full((d,), math.sqrt(d) / 4)
    ls = ls * (0.8 + 0.4 * torch.rand(d, generator=g0)) if ard else ls[:1]
    shift = X1.mean(0).to(dev)
    p1 = B.prep_points(kind, X1.to(dev), ls.to(dev), shift)
    p2 = p1 if m is None else B.prep_points(kind, X2.to(dev), ls.to(dev), shift)
    return p1, p2, g0


def _vectors(n, m, t, g0, symmetric):
    lt = 1 + 0.3 * torch.randn(t, n, generator=g0)
    rt = lt + 0.5 * torch.randn(t, n, generator=g0) if symmetric else 1 + 0.3 * torch.randn(t, m, generator=g0)
    return lt, rt


def _reference(kind, p1, p2, lt, rt):
    """(g float64 [1 + d], Gz1 float64 [n, d]); every sum is checked not to cancel."""
    d = p1.d
    z1, z2 = p1.xp[:, :d].double().cpu(), p2.xp[:, :d].double().cpu()
    W = lt.double().t() @ rt.double()
    s = torch.zeros(z1.shape[0], z2.shape[0], dtype=torch.float64)
    for q0 in range(0, d, 16):
        s += PR.sqdiff(z1[:, q0 : q0 + 16], z2[:, q0 : q0 + 16]).sum(-1)
    A = W * PR.dcov_ds(kind, s)
    Wk = W * PR.cov_s(kind, s)
    assert abs(float(Wk.sum())) >= 0.05 * float(Wk.abs().sum())
    g = [Wk.sum()]
    for q0 in range(0, d, 16):
        terms = A.unsqueeze(-1) * PR.sqdiff(z1[:, q0 : q0 + 16], z2[:, q0 : q0 + 16])
        sums = terms.sum((0, 1))
        assert bool((sums.abs() >= 0.05 * terms.abs().sum((0, 1))).all())
        g.extend(sums)
    gz = 2.0 * (z1 * A.sum(1, keepdim=True) - A @ z2)
    return torch.stack(g), gz


def _check(kind, p1, p2, lt, rt, mode, dev):
    from gpytorch_amd import backend as B

    assert B.wide_f32(p1, p2) and not p1.fused
    d = p1.d
    g_ref, gz_ref = _reference(kind, p1, p2, lt, rt)
    g, gz = B.kv_grad_wide(p1, p2, lt.to(dev), rt.to(dev), iso=mode == "iso", want_gz1=mode == "gz")
    g = g.double().cpu()
    print(kind, d, mode, "g0", float(g[0]), float(g_ref[0]))
    assert abs(float(g[0] - g_ref[0])) < BOUND * abs(float(g_ref[0]))
    if mode == "iso":
        assert gz is None and abs(float(g[1] - g_ref[1:].sum())) < BOUND * abs(float(g_ref[1:].sum()))
        assert bool((g[2:] == 0).all())
    else:
        err = ((g[1 : 1 + d] - g_ref[1:]).abs() / g_ref[1:].abs()).max()
        print("per-dimension", float(err))
        assert float(err) < BOUND
    if mode == "gz":
        print("gz1", rel_err(gz, gz_ref))
        assert gz.shape == gz_ref.shape and rel_err(gz, gz_ref) < BOUND
    return g, gz


# d: a chunk with one live dimension, whole chunks, one past a 64- and a 128-dimension block, the maximum; ragged tiles on both sides; t = 70: two passes
# of the W contraction; (640, 2048): several slabs
@pytest.mark.parametrize("kind,d,n,m,t,mode", [
    ("rbf", 33, 77, 131, 1, "iso"), ("matern32", 48, 333, 517, 11, "ard"), ("matern52", 129, 300, None, 33, "gz"), ("rbf", 512, 333, 517, 65, "ard"),
    ("matern52", 512, 300, None, 11, "gz"), ("matern32", 33, 333, 517, 65, "gz"), ("rbf", 129, 77, 131, 70, "ard"), ("matern52", 48, 300, None, 1, "iso"),
    ("matern32", 33, 640, 2048, 6, "gz"), ("rbf", 512, 77, 131, 33, "iso"), ("matern32", 129, 333, 517, 70, "gz"), ("rbf", 48, 300, None, 33, "gz")])
def test_sums_and_input_gradients(kind, d, n, m, t, mode, dev):
    p1, p2, g0 = _clouds(kind, d, n, m, dev, ard=mode != "iso")
    lt, rt = _vectors(n, m, t, g0, m is None)
    _check(kind, p1, p2, lt, rt, mode, dev)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [33, 512])
def test_at_the_norm_limit(kind, d, dev):
    """The four-cluster cloud of test_gpu_wide.py::test_at_the_norm_limit (|z|^2 = 25 .. 31): the cancellation case of the row-sum / column-sum
    expansion of the per-dimension sums and of Gz1 = 2 (z_i rs_i - u_i)."""
    from gpytorch_amd import backend as B

    n, t = 256, 11
    g0 = torch.Generator().manual_seed(0)
    c = torch.randn(4, d, generator=g0)
    c = c / c.norm(dim=1, keepdim=True) * math.sqrt(24.0)
    Z = c[torch.arange(n) % 4] + torch.randn(n, d, generator=g0) / math.sqrt(d)
    xp = B.prep_points(kind, (Z / B.prep_coef(kind)).float().to(dev), torch.ones(1, device=dev))
    assert 24.0 < xp.zmax2 <= B.WIDE_MAX_SQNORM
    lt, rt = _vectors(n, n, t, g0, True)
    _check(kind, xp, xp, lt, rt, "gz", dev)


def test_bitwise_reproducible(dev):
    from gpytorch_amd import backend as B

    p1, p2, g0 = _clouds("matern52", 129, 333, 517, dev, ard=True)
    lt, rt = (v.to(dev) for v in _vectors(333, 517, 33, g0, False))
    ga, za = B.kv_grad_wide(p1, p2, lt, rt, want_gz1=True)
    gb, zb = B.kv_grad_wide(p1, p2, lt, rt, want_gz1=True)
    assert torch.equal(ga, gb) and torch.equal(za, zb)


def test_routing_hyper_grads_with_input_gradients(dev):
    """d = 40 with want_x1 / want_x2 (refused before the wide derivative kernel) against float64 autograd through the dense kernel; with
    WIDE_KV = False the lengthscale and outputscale gradients come from the row-block path and agree."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    kind, n, m, d, t = "matern52", 300, 411, 40, 7
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
    assert B.wide_f32(p1, p2)
    out = hyper_grads(p1, p2, lsd, osd, lt.to(dev), rt.to(dev), want_x1=True, want_x2=True)
    for got, want in zip(out, ref):
        assert rel_err(got.reshape(want.shape), want) < BOUND
    B.WIDE_KV = False
    try:
        slow = hyper_grads(p1, p2, lsd, osd, lt.to(dev), rt.to(dev))
    finally:
        B.WIDE_KV = True
    assert rel_err(slow[0], out[0]) < BOUND and rel_err(slow[1], out[1]) < BOUND


def test_mll_backward_agrees_with_the_row_block_path(dev):
    """ExactMarginalLogLikelihood forward + backward at n = 2000, d = 64, ARD on the BBMM path with shared probes: finite gradients everywhere, the
    lengthscale gradient within 2e-3 (tests/test_gpu_highdim.py's BBMM figure) of the WIDE_KV = False run."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from tests.test_gpu_generic import _model

    n, d = 2000, 64
    X, y = make_data(n, d)
    Z = torch.randn(n, 10, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    grads = []
    for wide in (True, False):
        _, m, lik = _model("rbf", X, y, math.sqrt(d) / 4, 1.4, 0.1, dev, torch.float32, ard=True)
        mll = g.ExactMarginalLogLikelihood(lik, m)
        m.train(), lik.train()
        B.WIDE_KV = wide
        try:
            with g.settings.max_cholesky_size(0), g.settings.deterministic_probes(True):
                g.settings.deterministic_probes.probe_vectors = Z
                try:
                    mll(m(m.train_inputs[0]), m.train_targets).backward()
                finally:
                    g.settings.deterministic_probes.probe_vectors = None
        finally:
            B.WIDE_KV = True
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        grads.append(m.covar_module.base_kernel.raw_lengthscale.grad.clone())
    assert rel_err(grads[0], grads[1]) < 2e-3


@pytest.mark.parametrize("d,short,code", [(32, 0, "GPAMD_EINVAL"), (40, 1, "GPAMD_EWORKSPACE")])
def test_argument_errors(d, short, code, dev):
    """d below the envelope and a workspace one double short: the error code, and nothing written."""
    from gpytorch_amd import backend as B

    L, n, t = B.lib(), 200, 3
    p, _, g0 = _clouds("rbf", 40, n, None, dev, ard=False)
    z, nrm = B.wide_image(p)
    lt = torch.ones(t, n, device=dev)
    nd = int(L.gpamd_kv_wide_grad_workspace_doubles(n, n, 40, t, 0))
    ws = torch.full((nd,), 7.0, device=dev, dtype=torch.float64)
    out = torch.full((2 + p.dp,), 7.0, device=dev)
    wscale = torch.ones(2, device=dev)
    ptr = lambda v: C.c_void_p(v.data_ptr())
    rc = L.gpamd_kv_wide_grad_f32(B.kind_id(p), ptr(z), ptr(nrm), None, n, ptr(z), ptr(nrm), None, n, d, p.dp, ptr(lt), n, ptr(lt), n, t, 0, ptr(wscale),
                                  ptr(out), None, 0, ptr(ws), nd - short, None)
    codes = {"GPAMD_EINVAL": -1, "GPAMD_EWORKSPACE": -3}
    assert rc == codes[code] and bool((out == 7.0).all()) and bool((ws == 7.0).all())
