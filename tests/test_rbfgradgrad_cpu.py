"""CPU: the RBF kernel with first- and second-derivative observations off the device -- the reference's recorded values
(tests/golden/rbfgradgrad_values.npz, made by executing the reference's forward; square calls only: it fails for n1 != n2) against the float64
restatement (tests/rbfgradgrad_ref.py) and ``derivative.rbfgradgrad_dense``; rectangular inputs; the He_{s+2} + He_s identity of the lengthscale
derivative against autograd; the ``diag`` rule; ``kernels.rbfgradgrad_native``; ``means.ConstantMeanGradGrad``; the header; the C ABI's refusals
(before any launch: no device needed)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import rbfgradgrad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rbfgradgrad_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})


def _case(name):
    t = {k: torch.from_numpy(np.asarray(GOLD[f"{name}_{k}"])) for k in ("x1", "x2", "ls", "K")}
    return t, bool(GOLD[f"{name}_diag"])


def _same(t):
    return bool((t["x1"] == t["x2"]).all())


def _restated(t, diag):
    x1, x2, ls = t["x1"], t["x2"], t["ls"]
    if x1.dim() == 3:
        return torch.stack([R.dense(x1[b], x2[b], ls[b]) for b in range(x1.shape[0])])
    return R.diag(x1, ls) if diag else R.dense(x1, x2, ls)


def _tol(K):
    """1e-12 in float64; 1e-5 relative (to the largest entry) in float32."""
    return 1e-12 if K.dtype == torch.float64 else 1e-5 * float(K.abs().max())


def test_golden_covers_the_cases():
    seen = set()
    for name in CASES:
        t, diag = _case(name)
        assert t["x1"].shape == t["x2"].shape                    # the reference evaluates square calls only
        seen.add((t["x1"].shape[-1], _same(t), t["ls"].shape[-1] > 1, diag, t["K"].dtype, t["x1"].dim() == 3))
    assert {s[0] for s in seen} == {1, 2, 3, 4, 5}
    for i in (1, 2, 3, 5):      # same / different clouds, single / ARD, diag, a batch
        assert {s[i] for s in seen} == {False, True}, i
    assert {s[4] for s in seen} == {torch.float32, torch.float64}


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_golden(name):
    t, diag = _case(name)
    ref = _restated(t, diag)
    assert ref.shape == t["K"].shape
    err = float((ref - t["K"].double()).abs().max())
    assert err < _tol(t["K"]), (name, err)


@pytest.mark.parametrize("name", CASES)
def test_dense_form_and_kernel_class_equal_the_golden(name):
    """``rbfgradgrad_dense`` and what ``RBFKernelGradGrad`` returns off the device: ordering, ``diag``, batch, ``num_outputs_per_input``, dtype."""
    from gpytorch_amd.derivative import rbfgradgrad_dense
    from gpytorch_amd.kernels import RBFKernelGradGrad, rbfgradgrad_native
    from gpytorch_amd.operators import DenseLinearOperator

    t, diag = _case(name)
    x1, x2, ls, K = t["x1"], t["x2"], t["ls"], t["K"]
    d = x1.shape[-1]
    direct = rbfgradgrad_dense(x1, x2, ls, diag=diag)
    assert direct.shape == K.shape and direct.dtype == K.dtype
    assert float((direct.double() - K.double()).abs().max()) < _tol(K)
    kern = RBFKernelGradGrad(ard_num_dims=d if ls.shape[-1] > 1 else None, batch_shape=x1.shape[:-2]).to(K.dtype)
    kern.lengthscale = ls
    assert kern.num_outputs_per_input(x1, x2) == 2 * d + 1
    assert not rbfgradgrad_native(kern, x1, x2)                    # host tensors: the dense branch
    out = kern(x1, x1 if _same(t) else x2, diag=diag)
    if not diag:
        assert isinstance(out, DenseLinearOperator)
        out = out.to_dense()
    assert out.shape == K.shape and out.dtype == K.dtype
    assert float((out.detach().double() - K.double()).abs().max()) < _tol(K), name


@pytest.mark.parametrize("n,m,d,ard", [(7, 12, 1, True), (11, 6, 2, False), (5, 12, 3, True), (6, 9, 4, True), (4, 10, 5, False), (1, 3, 2, True)])
def test_rectangular_dense_form_equals_the_restatement(n, m, d, ard):
    """n1 != n2 -- the train x test block, which the reference cannot form -- in float64 (1e-12) and float32 (1e-5 relative); a batch as well."""
    from gpytorch_amd.derivative import rbfgradgrad_dense

    gen = torch.Generator().manual_seed(100 * n + m)
    x1, x2 = 2.0 * torch.rand(n, d, generator=gen, dtype=torch.float64), 2.0 * torch.rand(m, d, generator=gen, dtype=torch.float64)
    ls = 0.4 + 0.8 * torch.rand(1, d if ard else 1, generator=gen, dtype=torch.float64)
    ref = R.dense(x1, x2, ls)
    out = rbfgradgrad_dense(x1, x2, ls)
    assert out.shape == (n * (2 * d + 1), m * (2 * d + 1))
    assert float((out - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))
    out32 = rbfgradgrad_dense(x1.float(), x2.float(), ls.float())
    ref32 = R.dense(x1.float(), x2.float(), ls.float())
    assert out32.dtype == torch.float32 and float((out32.double() - ref32).abs().max()) < 1e-5 * float(ref32.abs().max())
    xb1, xb2 = torch.stack([x1, x1 + 0.1]), torch.stack([x2, x2 - 0.2])
    outb = rbfgradgrad_dense(xb1, xb2, ls)
    assert outb.shape == (2, *ref.shape) and float((outb[1] - R.dense(xb1[1], xb2[1], ls)).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))
    # the transposed matrix is the matrix of the exchanged clouds
    assert float((rbfgradgrad_dense(x2, x1, ls) - out.t()).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("d,ard", [(1, False), (2, True), (3, False), (3, True), (4, True)])
def test_lengthscale_derivative_is_the_shifted_hermite_block(d, ard):
    """autograd of ``rbfgradgrad_dense`` with respect to the lengthscale against the identity dK/dl_a = (1 / l_a) K with He_s(u_a) ->
    He_{s+2}(u_a) + He_s(u_a), and ``functions.rbfgrad_hyper_grads`` on the restatement's 1 + d sums (the convention of the fused kernel)."""
    from gpytorch_amd.derivative import rbfgradgrad_dense
    from gpytorch_amd.functions import rbfgrad_hyper_grads

    gen = torch.Generator().manual_seed(10 * d + ard)
    n, m, t = 9, 7, 3
    c = 2 * d + 1
    x1, x2 = torch.rand(n, d, generator=gen, dtype=torch.float64), torch.rand(m, d, generator=gen, dtype=torch.float64)
    ls = (0.3 + 0.5 * torch.rand(1, d if ard else 1, generator=gen, dtype=torch.float64)).requires_grad_(True)
    os_ = torch.tensor([1.3], dtype=torch.float64, requires_grad=True)
    L = torch.randn(n * c, t, generator=gen, dtype=torch.float64)
    Rv = torch.randn(m * c, t, generator=gen, dtype=torch.float64)
    val = (L * ((os_ * rbfgradgrad_dense(x1, x2, ls)) @ Rv)).sum()
    g_ls, g_os = torch.autograd.grad(val, [ls, os_])
    sums = R.sums(x1, x2, ls.detach(), L, Rv)
    d_ls, d_os = rbfgrad_hyper_grads(sums, ls.detach(), os_.detach())
    assert d_ls.shape == ls.shape and d_os.shape == os_.shape
    assert float((d_ls - g_ls).abs().max()) < 1e-10 * float(g_ls.abs().max())
    assert abs(float(d_os) - float(g_os)) < 1e-10 * abs(float(g_os))
    # entry by entry for one dimension under ARD: dK/dl_a = (1 / l_a) K^(a)
    if ard:
        lsa = ls.detach().clone().requires_grad_(True)
        K = rbfgradgrad_dense(x1, x2, lsa)
        W = torch.randn(K.shape, generator=gen, dtype=torch.float64)
        (gW,) = torch.autograd.grad((W * K).sum(), lsa)
        for a in range(d):
            want = (W * R.dense(x1, x2, ls.detach(), shifted=a)).sum() / ls.detach()[0, a]
            assert abs(float(gW[0, a]) - float(want)) < 1e-10 * max(1.0, abs(float(want)))


def test_diag_rule_and_kernel_class_surface():
    from gpytorch_amd.derivative import rbfgradgrad_dense
    from gpytorch_amd.kernels import RBFKernel, RBFKernelGradGrad, ScaleKernel

    gen = torch.Generator().manual_seed(1)
    x = torch.rand(5, 2, generator=gen, dtype=torch.float64)
    ls = torch.tensor([[0.4, 0.9]], dtype=torch.float64)
    dg = rbfgradgrad_dense(x, x, ls, diag=True)
    want = torch.tensor([1.0, 1 / 0.4 ** 2, 1 / 0.9 ** 2, 3 / 0.4 ** 4, 3 / 0.9 ** 4], dtype=torch.float64).repeat(5)
    assert dg.shape == (25,) and float((dg - want).abs().max()) < 1e-12
    assert float((dg - rbfgradgrad_dense(x, x, ls).diagonal()).abs().max()) < 1e-12
    assert float((dg - R.diag(x, ls)).abs().max()) < 1e-12
    with pytest.raises(RuntimeError, match="diag=True only works when x1 == x2"):
        rbfgradgrad_dense(x, x + 1.0, ls, diag=True)
    with pytest.raises(RuntimeError, match="diag=True only works when x1 == x2"):
        RBFKernelGradGrad()(x.float(), x.float()[:3], diag=True)
    assert not isinstance(RBFKernelGradGrad(), RBFKernel)         # (not a squared-exponential member of products)
    sk = ScaleKernel(RBFKernelGradGrad(ard_num_dims=2)).double()
    sk.outputscale, sk.base_kernel.lengthscale = 1.7, ls
    ref = 1.7 * R.dense(x, x, ls)
    assert float((sk(x).to_dense() - ref).abs().max()) < 1e-10
    assert float((sk(x, diag=True) - ref.diagonal()).abs().max()) < 1e-10
    rect = sk(x, x[:3] + 0.5).to_dense()                          # rectangular: what a posterior needs
    assert rect.shape == (25, 15) and float((rect - 1.7 * R.dense(x, x[:3] + 0.5, ls)).abs().max()) < 1e-10


def test_recognition_rule_table():
    """``rbfgradgrad_native``: float32, d <= 4, no batch, inputs without requires_grad, on the device.  It reads shapes, dtypes, ``requires_grad``
    and the device TYPE only, so a stand-in that carries those plays the device tensors here."""
    from gpytorch_amd.kernels import RBFKernelGradGrad, rbfgradgrad_native

    class Stub:
        def __init__(self, n, d, dtype=torch.float32, device="cuda", batch=(), requires_grad=False):
            self.shape, self.dtype, self.device, self.requires_grad = torch.Size([*batch, n, d]), dtype, torch.device(device), requires_grad

        def dim(self):
            return len(self.shape)

    dev = Stub
    k32, k64, kb = RBFKernelGradGrad(), RBFKernelGradGrad().double(), RBFKernelGradGrad(batch_shape=torch.Size([2]))
    for d in (1, 2, 3, 4):
        assert rbfgradgrad_native(k32, dev(9, d))
        assert rbfgradgrad_native(k32, dev(9, d), dev(5, d))
        assert rbfgradgrad_native(RBFKernelGradGrad(ard_num_dims=d), dev(9, d))
    assert not rbfgradgrad_native(k32, dev(9, 5))                                   # d > 4
    assert not rbfgradgrad_native(k32, dev(9, 2, dtype=torch.float64))              # float64 inputs
    assert not rbfgradgrad_native(k64, dev(9, 2))                                   # float64 parameters
    assert not rbfgradgrad_native(kb, dev(9, 2))                                    # a batch of kernels
    assert not rbfgradgrad_native(k32, dev(9, 2, batch=(3,)))                       # a batch of inputs
    assert not rbfgradgrad_native(k32, dev(9, 2), dev(5, 2, batch=(3,)))
    assert not rbfgradgrad_native(k32, dev(9, 2), last_dim_is_batch=True)
    assert not rbfgradgrad_native(k32, dev(9, 2, requires_grad=True))               # input gradients
    assert not rbfgradgrad_native(k32, dev(9, 2), dev(5, 2, requires_grad=True))
    assert not rbfgradgrad_native(k32, dev(9, 2, device="cpu"))                     # host tensors
    assert not rbfgradgrad_native(k32, dev(9, 2), dev(5, 2, device="cpu"))


def test_constant_mean_gradgrad():
    from gpytorch_amd.means import ConstantMeanGrad, ConstantMeanGradGrad

    m = ConstantMeanGradGrad()
    assert m.constant.shape == (1,)
    with torch.no_grad():
        m.constant.fill_(1.5)
    out = m(torch.rand(7, 3))
    assert out.shape == (7, 7)
    assert torch.equal(out[:, 0], torch.full((7,), 1.5)) and torch.equal(out[:, 1:], torch.zeros(7, 6))
    out.sum().backward()
    assert float(m.constant.grad) == 7.0                                            # only the value column depends on the constant
    assert m(torch.rand(2, 5, 3)).shape == (2, 5, 7)
    mb = ConstantMeanGradGrad(batch_shape=torch.Size([2]))
    with torch.no_grad():
        mb.constant.copy_(torch.tensor([[1.0], [2.0]]))
    outb = mb(torch.rand(2, 5, 3))
    assert outb.shape == (2, 5, 7) and torch.equal(outb[..., 0], torch.tensor([[1.0] * 5, [2.0] * 5])) and not outb[..., 1:].any()
    assert m(torch.rand(6)).shape == (6, 3)                                         # 1-D inputs are [n, 1]
    assert ConstantMeanGrad()(torch.rand(7, 3)).shape == (7, 4)                     # the first-order mean keeps its d + 1 columns


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    hdr = open(os.path.join(ROOT, "include", "gpamd.h")).read()
    assert re.search(r"#define\s+GPAMD_ABI_VERSION\s+5\b", hdr)
    for name in ("plan", "partials_f32", "grad_workspace_doubles", "grad_f32"):
        assert re.search(r"\bgpamd_kv_rbfgradgrad_%s\s*\(" % name, hdr), name
    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5
    for name in ("plan", "partials_f32", "grad_workspace_doubles", "grad_f32"):
        assert hasattr(h, f"gpamd_kv_rbfgradgrad_{name}")


def test_entry_points_refuse_bad_arguments_without_gpu():
    import ctypes

    from gpytorch_amd._lib import lib

    h = lib()
    raw = ctypes.create_string_buffer(256)
    buf = (ctypes.addressof(raw) + 15) // 16 * 16      # (non-null, 16-byte aligned host address: never dereferenced before the checks)
    S, jc, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    # plan: d = 3 -> 7 components per point
    assert h.gpamd_kv_rbfgradgrad_plan(1000, 1000, 5, 4, 11000, S, jc, ws) == -2 and b"d must be in 1..4" in h.gpamd_last_error()
    assert h.gpamd_kv_rbfgradgrad_plan(1000, 1000, 0, 4, 11000, S, jc, ws) == -2
    assert h.gpamd_kv_rbfgradgrad_plan(1000, 1000, 3, 4, 6999, S, jc, ws) == -1 and h.gpamd_last_error().startswith(b"kv_rbfgradgrad_plan:")
    assert b"2 d + 1" in h.gpamd_last_error()
    assert h.gpamd_kv_rbfgradgrad_plan(0, 1000, 3, 4, 7000, S, jc, ws) == -1
    for n, m, d, t in [(1, 1, 1, 1), (7, 5, 2, 3), (1025, 257, 3, 11), (20_000, 20_000, 3, 11), (300, 100_000, 4, 5)]:
        ldo = (n * (2 * d + 1) + 3) // 4 * 4
        assert h.gpamd_kv_rbfgradgrad_plan(n, m, d, t, ldo, S, jc, ws) == 0
        assert S.value >= 1 and jc.value % 256 == 0 and S.value * jc.value >= m and (S.value - 1) * jc.value < m
        assert ws.value == S.value * t * ldo
    # product: d outside 1..4, null pointers, short leading dimensions, a chunk that is not the plan's -- all before any launch
    ok = dict(inv=buf, d=3, x1=buf, n=10, x2=buf, m=12, vt=buf, ldv=84, t=2, p=buf, ldo=70, S=1, jc=256)

    def kv(**kw):
        a = dict(ok, **kw)
        return h.gpamd_kv_rbfgradgrad_partials_f32(a["inv"], a["d"], a["x1"], a["n"], a["x2"], a["m"], a["vt"], a["ldv"], a["t"], a["p"], a["ldo"], a["S"],
                                                   a["jc"], None, None)

    assert kv(d=5) == -2 and kv(d=0) == -2 and h.gpamd_last_error().startswith(b"kv_rbfgradgrad:")
    for name in ("inv", "x1", "x2", "vt", "p"):
        assert kv(**{name: None}) == -1 and b"null pointer" in h.gpamd_last_error(), name
    assert kv(ldv=83) == -1 and b"leading dimensions" in h.gpamd_last_error()
    assert kv(ldo=69) == -1 and b"leading dimensions" in h.gpamd_last_error()
    assert kv(ldv=48, ldo=40) == -1                                                 # (what the first-order entry point accepts is too short here)
    assert kv(jc=100) == -1 and b"jchunk" in h.gpamd_last_error()
    assert kv(jc=0) == -1 and kv(S=0) == -1
    assert kv(m=300, ldv=2100, jc=256, S=1) == -1 and b"jchunk" in h.gpamd_last_error()   # a chunk that does not cover m
    assert kv(n=0) == -1 and kv(t=0) == -1
    # derivative
    okg = dict(inv=buf, d=3, x1=buf, n=10, x2=buf, m=12, lt=buf, ldl=70, rt=buf, ldr=84, t=2, out=buf, ws=buf, nws=1 << 20)

    def grad(**kw):
        a = dict(okg, **kw)
        return h.gpamd_kv_rbfgradgrad_grad_f32(a["inv"], a["d"], a["x1"], a["n"], a["x2"], a["m"], a["lt"], a["ldl"], a["rt"], a["ldr"], a["t"], a["out"],
                                               a["ws"], a["nws"], None)

    assert grad(d=5) == -2 and grad(d=0) == -2 and h.gpamd_last_error().startswith(b"kv_rbfgradgrad_grad:")
    for name in ("inv", "x1", "x2", "lt", "rt", "out", "ws"):
        assert grad(**{name: None}) == -1 and b"null pointer" in h.gpamd_last_error(), name
    assert grad(ldl=69) == -1 and grad(ldr=83) == -1 and b"leading dimensions" in h.gpamd_last_error()
    need = h.gpamd_kv_rbfgradgrad_grad_workspace_doubles(10, 12, 3)
    assert need >= 4 and h.gpamd_kv_rbfgradgrad_grad_workspace_doubles(10, 12, 5) == 0
    assert grad(nws=need - 1) == -3 and h.gpamd_last_error().startswith(b"kv_rbfgradgrad_grad:")


def test_operator_dense_algebra_off_the_device():
    """The parts of ``RBFGradGradFusedLinearOperator`` that launch nothing: sizes, ``to_dense``, ``diagonal``, point-aligned slices, ``+ diag`` and
    the Cholesky branch of ``inv_quad_logdet`` with its autograd path to the lengthscale, the outputscale and a per-entry noise vector."""
    from gpytorch_amd.derivative import RBFGradGradFusedAddedDiagLinearOperator, RBFGradGradFusedLinearOperator
    from gpytorch_amd.operators import DenseLinearOperator, DiagLinearOperator

    gen = torch.Generator().manual_seed(9)
    n, m, d = 8, 5, 2
    c = 2 * d + 1
    x, x2 = torch.rand(n, d, generator=gen, dtype=torch.float64) + 1000.0, torch.rand(m, d, generator=gen, dtype=torch.float64) + 1000.0
    ls = torch.tensor([[0.4, 0.7]], dtype=torch.float64, requires_grad=True)
    os_ = torch.tensor([1.7], dtype=torch.float64, requires_grad=True)
    op, rect = RBFGradGradFusedLinearOperator(x, x, ls, os_), RBFGradGradFusedLinearOperator(x, x2, ls, os_)
    assert op.family == "rbf" and op.order == 2
    Kref, Krect = 1.7 * R.dense(x, x, ls.detach()), 1.7 * R.dense(x, x2, ls.detach())
    scale = float(Kref.abs().max())
    assert op.shape == (n * c, n * c) and rect.shape == (n * c, m * c) and rect.mT.shape == (m * c, n * c)
    assert float((op.to_dense() - Kref).abs().max()) < 1e-9 * scale               # (coordinates near 1000: the operator centres them)
    assert float((rect.mT.to_dense() - Krect.t()).abs().max()) < 1e-9 * scale
    assert float((op.diagonal() - Kref.diagonal()).abs().max()) < 1e-12 * scale
    sub = rect[c : 4 * c, 2 * c :]
    assert isinstance(sub, RBFGradGradFusedLinearOperator) and float((sub.to_dense() - Krect[c : 4 * c, 2 * c :]).abs().max()) < 1e-9 * scale
    assert isinstance(rect[1:4, :], DenseLinearOperator)
    assert isinstance(rect[d + 1 : 2 * (d + 1), :], DenseLinearOperator)          # (aligned to d + 1, not to 2 d + 1: cuts through a point)
    assert op.mul(2.0).outputscale.shape == (1,) and float((op.mul(2.0).to_dense() - 2.0 * Kref).abs().max()) < 1e-9 * scale
    noise = (0.05 + 0.1 * torch.rand(n * c, generator=gen, dtype=torch.float64)).requires_grad_(True)
    added = op + DiagLinearOperator(noise)
    assert isinstance(added, RBFGradGradFusedAddedDiagLinearOperator)
    y = torch.randn(n * c, generator=gen, dtype=torch.float64)
    iq, ld = added.inv_quad_logdet(y, logdet=True)                                # n (2 d + 1) = 40 <= max_cholesky_size: the Cholesky branch
    got = torch.autograd.grad(iq + ld, [ls, os_, noise])
    ls2, os2, nz2 = (t.detach().clone().requires_grad_(True) for t in (ls, os_, noise))
    Kh = os2 * R.dense(x, x, ls2) + torch.diag(nz2)
    want = torch.autograd.grad(y @ torch.linalg.solve(Kh, y) + torch.logdet(Kh), [ls2, os2, nz2])
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) < 1e-7 * float(b.abs().max())


def test_model_with_second_derivatives_off_the_device():
    """ExactGP + ``ConstantMeanGradGrad`` + ``MultitaskGaussianLikelihood(num_tasks=3)`` in float64 (the dense branch): the posterior over a
    RECTANGULAR train x test block, and a fantasy model against a model conditioned on the concatenated data."""
    import math

    import gpytorch_amd as g

    gen = torch.Generator().manual_seed(4)
    w = 2 * math.pi

    def targets(x):
        return torch.hstack([torch.sin(w * x), w * torch.cos(w * x), -w * w * torch.sin(w * x)])

    tx = torch.linspace(0, 1, 15, dtype=torch.float64).reshape(-1, 1)
    nx = torch.rand(4, 1, generator=gen, dtype=torch.float64)
    xs = torch.rand(9, 1, generator=gen, dtype=torch.float64)

    def build(x, y):
        class GPWithSecondDerivatives(g.models.ExactGP):
            def __init__(self, x_, y_, lik_):
                super().__init__(x_, y_, lik_)
                self.mean_module = g.means.ConstantMeanGradGrad()
                self.covar_module = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad())

            def forward(self, x_):
                return g.distributions.MultitaskMultivariateNormal(self.mean_module(x_), self.covar_module(x_))

        mod = GPWithSecondDerivatives(x, y, g.likelihoods.MultitaskGaussianLikelihood(num_tasks=3).double()).double()
        mod.covar_module.base_kernel.lengthscale = 0.3
        mod.eval()
        mod.likelihood.eval()
        return mod

    with torch.no_grad():
        model = build(tx, targets(tx))
        mu = model(xs).mean
        assert mu.shape == (9, 3)
        assert float((mu[:, 0] - torch.sin(w * xs[:, 0])).abs().max()) < 0.2     # the value is interpolated from 15 x 3 observations
        fant = model.get_fantasy_model(nx, targets(nx))
        assert fant.train_targets.shape == (19, 3)
        mu_f, mu_c = fant(xs).mean, build(torch.cat([tx, nx]), torch.cat([targets(tx), targets(nx)]))(xs).mean
    assert mu_f.shape == (9, 3) and float((mu_f - mu_c).abs().max()) < 1e-6 * float(mu_c.abs().max())
