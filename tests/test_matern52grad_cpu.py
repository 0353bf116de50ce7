"""CPU: the Matern-5/2 kernel with derivative observations off the device -- the reference's recorded values (tests/golden/matern52grad_values.npz,
made by executing the reference's forward) against the float64 restatement (tests/matern52grad_ref.py) and the kernel class's dense branch; the
class surface; the recognition rule ``kernels.matern52grad_native``; input gradients of the dense branch, finite at coincident points; the host
assembly of the hyper-gradients from the 1 + d sums against autograd; the C ABI's refusals (before any launch: no device needed); the operator's
dense algebra and a fantasy model."""
import math
import os

import numpy as np
import pytest
import torch

from tests import matern52grad_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matern52grad_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})


def _case(name):
    t = {k: torch.from_numpy(np.asarray(GOLD[f"{name}_{k}"])) for k in ("x1", "x2", "ls", "K")}
    return t, bool(GOLD[f"{name}_diag"])


def _same(t):
    return t["x1"].shape == t["x2"].shape and bool((t["x1"] == t["x2"]).all())


def _restated(t, diag):
    x1, x2, ls = t["x1"], t["x2"], t["ls"]
    if x1.dim() == 3:
        return torch.stack([R.dense(x1[b], x2[b], ls[b]) for b in range(x1.shape[0])])
    return R.diag(x1, ls) if diag else R.dense(x1, x2, ls)


def test_golden_covers_the_cases():
    seen = set()
    for name in CASES:
        t, diag = _case(name)
        seen.add((t["x1"].shape[-1], _same(t), t["ls"].shape[-1] > 1, diag, t["K"].dtype, t["x1"].dim() == 3))
        assert max(t["x1"].shape[-2], t["x2"].shape[-2]) <= 12
    assert {s[0] for s in seen} == {1, 2, 3, 4, 5}
    for i in (1, 2, 3, 5):      # square / rectangular, single / ARD, diag, float32 / float64, a batch
        assert {s[i] for s in seen} == {False, True}, i
    assert {s[4] for s in seen} == {torch.float32, torch.float64}


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_golden(name):
    t, diag = _case(name)
    ref = _restated(t, diag)
    assert ref.shape == t["K"].shape
    err = float((ref - t["K"].double()).abs().max())
    assert err < (1e-12 if t["K"].dtype == torch.float64 else 1e-5), (name, err)


@pytest.mark.parametrize("name", CASES)
def test_kernel_class_dense_branch_equals_the_golden(name):
    """Ordering, ``diag``, batch, ``num_outputs_per_input`` and dtype of what ``Matern52KernelGrad`` returns off the device."""
    from gpytorch_amd.kernels import Matern52KernelGrad, matern52grad_native
    from gpytorch_amd.operators import DenseLinearOperator

    t, diag = _case(name)
    x1, x2, ls, K = t["x1"], t["x2"], t["ls"], t["K"]
    d = x1.shape[-1]
    kern = Matern52KernelGrad(ard_num_dims=d if ls.shape[-1] > 1 else None, batch_shape=x1.shape[:-2]).to(K.dtype)
    kern.lengthscale = ls
    assert kern.num_outputs_per_input(x1, x2) == d + 1
    assert not matern52grad_native(kern, x1, x2)                       # host tensors: the dense branch
    out = kern(x1, x1 if _same(t) else x2, diag=diag)
    if not diag:
        assert isinstance(out, DenseLinearOperator)
        out = out.to_dense()
    assert out.shape == K.shape and out.dtype == K.dtype
    err = float((out.double() - K.double()).abs().max())
    assert err < (1e-12 if K.dtype == torch.float64 else 1e-5), (name, err)


def test_kernel_class_surface():
    from gpytorch_amd.kernels import Matern52KernelGrad, ScaleKernel

    assert Matern52KernelGrad(nu=1.5).nu == 2.5                                 # a ``nu`` keyword is accepted and dropped, as in the reference
    kernel = Matern52KernelGrad()
    kernel.initialize(lengthscale=3.14)
    assert float(torch.norm(kernel.lengthscale - torch.tensor(3.14).view_as(kernel.lengthscale))) < 1e-5
    kernel = Matern52KernelGrad(batch_shape=torch.Size([2]))
    ls_init = torch.tensor([3.14, 4.13])
    kernel.initialize(lengthscale=ls_init)
    assert float(torch.norm(kernel.lengthscale - ls_init.view_as(kernel.lengthscale))) < 1e-5
    # diag=True of two different inputs is an error, as in the reference
    x = torch.rand(5, 2)
    with pytest.raises(RuntimeError, match="diag=True only works when x1 == x2"):
        Matern52KernelGrad()(x, x + 1.0, diag=True)
    # under ScaleKernel: the outputscale multiplies everything, the diagonal included
    sk = ScaleKernel(Matern52KernelGrad(ard_num_dims=2))
    sk.outputscale, sk.base_kernel.lengthscale = 1.7, torch.tensor([[0.4, 0.9]])
    ref = 1.7 * R.dense(x, x, torch.tensor([0.4, 0.9]))
    assert float((sk(x).to_dense().double() - ref).abs().max()) < 1e-5
    assert float((sk(x, diag=True).double() - ref.diagonal()).abs().max()) < 1e-5
    # last_dim_is_batch: every dimension becomes a batch member of one-dimensional kernels, as the reference's __call__ arranges it
    k1 = Matern52KernelGrad()
    k1.lengthscale = 0.6
    out = k1(x, last_dim_is_batch=True).to_dense()
    assert out.shape == (2, 10, 10)
    for j in range(2):
        assert float((out[j].double() - R.dense(x[:, j : j + 1], x[:, j : j + 1], torch.tensor([0.6]))).abs().max()) < 1e-5


def test_recognition_rule_table():
    """``matern52grad_native``: float32, d <= 4, no batch, inputs without requires_grad, on the device.  It reads shapes, dtypes, ``requires_grad`` and
    the device TYPE only, so a stand-in that carries those plays the device tensors here."""
    from gpytorch_amd.kernels import Matern52KernelGrad, matern52grad_native

    class Stub:
        def __init__(self, n, d, dtype=torch.float32, device="cuda", batch=(), requires_grad=False):
            self.shape, self.dtype, self.device, self.requires_grad = torch.Size([*batch, n, d]), dtype, torch.device(device), requires_grad

        def dim(self):
            return len(self.shape)

    dev = Stub
    k32, k64, kb = Matern52KernelGrad(), Matern52KernelGrad().double(), Matern52KernelGrad(batch_shape=torch.Size([2]))
    for d in (1, 2, 3, 4):
        assert matern52grad_native(k32, dev(9, d))
        assert matern52grad_native(k32, dev(9, d), dev(5, d))
        assert matern52grad_native(Matern52KernelGrad(ard_num_dims=d), dev(9, d))
    assert not matern52grad_native(k32, dev(9, 5))                                   # d > 4
    assert not matern52grad_native(k32, dev(9, 2, dtype=torch.float64))              # float64 inputs
    assert not matern52grad_native(k64, dev(9, 2))                                   # float64 parameters
    assert not matern52grad_native(kb, dev(9, 2))                                    # a batch of kernels
    assert not matern52grad_native(k32, dev(9, 2, batch=(3,)))                       # a batch of inputs
    assert not matern52grad_native(k32, dev(9, 2), dev(5, 2, batch=(3,)))
    assert not matern52grad_native(k32, dev(9, 2), last_dim_is_batch=True)
    assert not matern52grad_native(k32, dev(9, 2, requires_grad=True))               # input gradients
    assert not matern52grad_native(k32, dev(9, 2), dev(5, 2, requires_grad=True))
    assert not matern52grad_native(k32, dev(9, 2, device="cpu"))                     # host tensors
    assert not matern52grad_native(k32, dev(9, 2), dev(5, 2, device="cpu"))


def test_dense_branch_carries_input_gradients():
    """What the rule declines stays differentiable with respect to the inputs (plain autograd through ``matern52grad_dense``)."""
    from gpytorch_amd.kernels import Matern52KernelGrad

    gen = torch.Generator().manual_seed(3)
    x = torch.rand(6, 2, generator=gen, dtype=torch.float64, requires_grad=True)
    kern = Matern52KernelGrad().double()
    W = torch.randn(18, 18, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad((W * kern(x).to_dense()).sum(), x)
    x2 = x.detach().clone().requires_grad_(True)
    (gref,) = torch.autograd.grad((W * R.dense(x2, x2, kern.lengthscale.detach())).sum(), x2)
    assert float((gx - gref).abs().max()) < 1e-10 * float(gref.abs().max())


def test_dense_branch_is_finite_at_coincident_points():
    """x1 == x2 puts s = 0 on every diagonal pair: the matrix, its input gradients and its lengthscale gradient stay finite, in both dtypes (the
    square root carries an epsilon), and the diagonal blocks are [[1, 0], [0, (5/3) / l^2]]."""
    from gpytorch_amd.derivative import matern52grad_dense

    for dt in (torch.float64, torch.float32):
        gen = torch.Generator().manual_seed(8)
        x = torch.rand(5, 3, generator=gen, dtype=dt)
        x = torch.cat([x, x[:2]]).requires_grad_(True)              # two repeated points: off-diagonal coincidences too
        ls = torch.tensor([[0.4, 0.7, 0.5]], dtype=dt, requires_grad=True)
        K = matern52grad_dense(x, x, ls)
        W = torch.randn(K.shape, generator=gen, dtype=dt)
        gx, gl = torch.autograd.grad((W * K).sum(), [x, ls])
        assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gl).all())
        blk = K.detach()[:4, :4].double()
        want = torch.diag(torch.cat([torch.ones(1, dtype=torch.float64), (5.0 / 3.0) / ls.detach().double().reshape(-1).pow(2)]))
        assert float((blk - want).abs().max()) < (1e-9 if dt == torch.float64 else 1e-5)
        assert float((K.detach().double() - R.dense(x.detach(), x.detach(), ls.detach())).abs().max()) < (1e-9 if dt == torch.float64 else 2e-5)


@pytest.mark.parametrize("d,ard", [(1, False), (2, True), (3, False), (3, True), (4, True)])
def test_hyper_gradient_assembly_matches_autograd(d, ard):
    """``functions.rbfgrad_hyper_grads`` (it serves both families) on the 1 + d sums (computed here in torch float64) against autograd through the dense matrix, 1e-10."""
    from gpytorch_amd.functions import rbfgrad_hyper_grads

    gen = torch.Generator().manual_seed(10 * d + ard)
    n, m, t = 9, 7, 3
    x1, x2 = torch.rand(n, d, generator=gen, dtype=torch.float64), torch.rand(m, d, generator=gen, dtype=torch.float64)
    ls = (0.3 + 0.5 * torch.rand(1, d if ard else 1, generator=gen, dtype=torch.float64)).requires_grad_(True)
    os_ = torch.tensor([1.3], dtype=torch.float64, requires_grad=True)
    L = torch.randn(n * (d + 1), t, generator=gen, dtype=torch.float64)
    Rv = torch.randn(m * (d + 1), t, generator=gen, dtype=torch.float64)
    val = (L * ((os_ * R.dense(x1, x2, ls)) @ Rv)).sum()
    g_ls, g_os = torch.autograd.grad(val, [ls, os_])
    sums = R.sums(x1, x2, ls.detach(), L, Rv)
    d_ls, d_os = rbfgrad_hyper_grads(sums, ls.detach(), os_.detach())
    assert d_ls.shape == ls.shape and d_os.shape == os_.shape
    assert float((d_ls - g_ls).abs().max()) < 1e-10 * float(g_ls.abs().max())
    assert abs(float(d_os) - float(g_os)) < 1e-10 * abs(float(g_os))
    d_ls1, d_none = rbfgrad_hyper_grads(sums, ls.detach(), None)                # no ScaleKernel: outputscale 1, no gradient slot
    assert d_none is None and float((d_ls1 * 1.3 - g_ls).abs().max()) < 1e-10 * float(g_ls.abs().max())


def test_entry_points_refuse_bad_arguments_without_gpu():
    import ctypes

    from gpytorch_amd._lib import lib

    h = lib()
    raw = ctypes.create_string_buffer(256)
    buf = (ctypes.addressof(raw) + 15) // 16 * 16      # (non-null, 16-byte aligned host address: never dereferenced before the checks)
    S, jc, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    # plan
    assert h.gpamd_kv_m52grad_plan(1000, 1000, 5, 4, 6000, S, jc, ws) == -2 and b"d must be in 1..4" in h.gpamd_last_error()
    assert h.gpamd_kv_m52grad_plan(1000, 1000, 0, 4, 6000, S, jc, ws) == -2
    assert h.gpamd_kv_m52grad_plan(1000, 1000, 3, 4, 3999, S, jc, ws) == -1 and h.gpamd_last_error().startswith(b"kv_m52grad_plan:")
    assert h.gpamd_kv_m52grad_plan(0, 1000, 3, 4, 4000, S, jc, ws) == -1
    for n, m, d, t in [(1, 1, 1, 1), (7, 5, 2, 3), (1025, 257, 3, 11), (20_000, 20_000, 3, 11), (300, 100_000, 4, 5)]:
        ldo = (n * (d + 1) + 3) // 4 * 4
        assert h.gpamd_kv_m52grad_plan(n, m, d, t, ldo, S, jc, ws) == 0
        assert S.value >= 1 and jc.value % 256 == 0 and S.value * jc.value >= m and (S.value - 1) * jc.value < m
        assert ws.value == S.value * t * ldo
    # product: d outside 1..4, null pointers, short leading dimensions, a chunk that is not the plan's -- all before any launch
    ok = dict(inv=buf, d=3, x1=buf, n=10, x2=buf, m=12, vt=buf, ldv=48, t=2, p=buf, ldo=40, S=1, jc=256)

    def kv(**kw):
        a = dict(ok, **kw)
        return h.gpamd_kv_m52grad_partials_f32(a["inv"], a["d"], a["x1"], a["n"], a["x2"], a["m"], a["vt"], a["ldv"], a["t"], a["p"], a["ldo"], a["S"],
                                               a["jc"], None, None)

    assert kv(d=5) == -2 and kv(d=0) == -2 and h.gpamd_last_error().startswith(b"kv_m52grad:")
    for name in ("inv", "x1", "x2", "vt", "p"):
        assert kv(**{name: None}) == -1 and b"null pointer" in h.gpamd_last_error(), name
    assert kv(ldv=47) == -1 and b"leading dimensions" in h.gpamd_last_error()
    assert kv(ldo=39) == -1 and b"leading dimensions" in h.gpamd_last_error()
    assert kv(jc=100) == -1 and b"jchunk" in h.gpamd_last_error()
    assert kv(n=0) == -1 and kv(t=0) == -1
    # derivative
    okg = dict(inv=buf, d=3, x1=buf, n=10, x2=buf, m=12, lt=buf, ldl=40, rt=buf, ldr=48, t=2, out=buf, ws=buf, nws=1 << 20)

    def grad(**kw):
        a = dict(okg, **kw)
        return h.gpamd_kv_m52grad_grad_f32(a["inv"], a["d"], a["x1"], a["n"], a["x2"], a["m"], a["lt"], a["ldl"], a["rt"], a["ldr"], a["t"], a["out"],
                                           a["ws"], a["nws"], None)

    assert grad(d=5) == -2 and grad(d=0) == -2 and h.gpamd_last_error().startswith(b"kv_m52grad_grad:")
    for name in ("inv", "x1", "x2", "lt", "rt", "out", "ws"):
        assert grad(**{name: None}) == -1 and b"null pointer" in h.gpamd_last_error(), name
    assert grad(ldl=39) == -1 and grad(ldr=47) == -1 and b"leading dimensions" in h.gpamd_last_error()
    need = h.gpamd_kv_m52grad_grad_workspace_doubles(10, 12, 3)
    assert need >= 4 and h.gpamd_kv_m52grad_grad_workspace_doubles(10, 12, 5) == 0
    assert grad(nws=need - 1) == -3 and h.gpamd_last_error().startswith(b"kv_m52grad_grad:")


def test_operator_dense_algebra_off_the_device():
    """The parts of ``Matern52GradFusedLinearOperator`` that launch nothing: sizes, ``to_dense``, ``diagonal``, point-aligned slices, ``+ diag`` and the
    Cholesky branch of ``inv_quad_logdet`` with its autograd path to the lengthscale, the outputscale and a per-entry noise vector."""
    from gpytorch_amd.derivative import Matern52GradFusedAddedDiagLinearOperator, Matern52GradFusedLinearOperator
    from gpytorch_amd.operators import DenseLinearOperator, DiagLinearOperator

    gen = torch.Generator().manual_seed(9)
    n, m, d = 8, 5, 2
    c = d + 1
    x, x2 = torch.rand(n, d, generator=gen, dtype=torch.float64) + 1000.0, torch.rand(m, d, generator=gen, dtype=torch.float64) + 1000.0
    ls = torch.tensor([[0.4, 0.7]], dtype=torch.float64, requires_grad=True)
    os_ = torch.tensor([1.7], dtype=torch.float64, requires_grad=True)
    op, rect = Matern52GradFusedLinearOperator(x, x, ls, os_), Matern52GradFusedLinearOperator(x, x2, ls, os_)
    Kref, Krect = 1.7 * R.dense(x, x, ls.detach()), 1.7 * R.dense(x, x2, ls.detach())
    assert op.shape == (n * c, n * c) and rect.shape == (n * c, m * c) and rect.mT.shape == (m * c, n * c)
    assert float((op.to_dense() - Kref).abs().max()) < 1e-9                      # (coordinates near 1000: the operator centres them)
    assert float((rect.mT.to_dense() - Krect.t()).abs().max()) < 1e-9
    assert float((op.diagonal() - Kref.diagonal()).abs().max()) < 1e-12
    sub = rect[c : 4 * c, 2 * c :]
    assert isinstance(sub, Matern52GradFusedLinearOperator) and float((sub.to_dense() - Krect[c : 4 * c, 2 * c :]).abs().max()) < 1e-9
    assert isinstance(rect[1:4, :], DenseLinearOperator)
    assert op.mul(2.0).outputscale.shape == (1,) and float((op.mul(2.0).to_dense() - 2.0 * Kref).abs().max()) < 1e-9
    noise = (0.05 + 0.1 * torch.rand(n * c, generator=gen, dtype=torch.float64)).requires_grad_(True)
    added = op + DiagLinearOperator(noise)
    assert isinstance(added, Matern52GradFusedAddedDiagLinearOperator)
    y = torch.randn(n * c, generator=gen, dtype=torch.float64)
    iq, ld = added.inv_quad_logdet(y, logdet=True)                              # n (d + 1) = 24 <= max_cholesky_size: the Cholesky branch
    got = torch.autograd.grad(iq + ld, [ls, os_, noise])
    ls2, os2, nz2 = (t.detach().clone().requires_grad_(True) for t in (ls, os_, noise))
    Kh = os2 * R.dense(x, x, ls2) + torch.diag(nz2)
    want = torch.autograd.grad(y @ torch.linalg.solve(Kh, y) + torch.logdet(Kh), [ls2, os2, nz2])
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) < 1e-7 * float(b.abs().max())


def test_fantasy_model_of_a_derivative_gp_off_the_device():
    """``get_fantasy_model`` with multitask targets [m, d + 1] (float64, the dense branch): its mean equals that of a model conditioned on the
    concatenated data."""
    import gpytorch_amd as g

    gen = torch.Generator().manual_seed(4)
    tx = torch.linspace(0, 1, 15, dtype=torch.float64).reshape(-1, 1)
    ty = torch.hstack([torch.sin(2 * math.pi * tx), 2 * math.pi * torch.cos(2 * math.pi * tx)])
    nx, ny = torch.rand(4, 1, generator=gen, dtype=torch.float64), torch.randn(4, 2, generator=gen, dtype=torch.float64)
    xs = torch.rand(9, 1, generator=gen, dtype=torch.float64)

    def build(x, y):
        class GPWithDerivatives(g.models.ExactGP):
            def __init__(self, x_, y_, lik_):
                super().__init__(x_, y_, lik_)
                self.mean_module = g.means.ConstantMeanGrad()
                self.covar_module = g.kernels.ScaleKernel(g.kernels.Matern52KernelGrad())

            def forward(self, x_):
                return g.distributions.MultitaskMultivariateNormal(self.mean_module(x_), self.covar_module(x_))

        mod = GPWithDerivatives(x, y, g.likelihoods.MultitaskGaussianLikelihood(num_tasks=2).double()).double()
        mod.covar_module.base_kernel.lengthscale = 0.3
        mod.eval()
        mod.likelihood.eval()
        return mod

    with torch.no_grad():
        model = build(tx, ty)
        with pytest.raises(RuntimeError, match="Fantasy observations can only be added after making predictions"):
            model.get_fantasy_model(nx, ny)
        model(xs)
        with pytest.raises(NotImplementedError):
            model.get_fantasy_model(nx, ny.reshape(-1))                         # multitask targets are [m, T]
        fant = model.get_fantasy_model(nx, ny)
        assert fant.train_targets.shape == (19, 2)
        mu_f, mu_c = fant(xs).mean, build(torch.cat([tx, nx]), torch.cat([ty, ny]))(xs).mean
    assert mu_f.shape == (9, 2) and float((mu_f - mu_c).abs().max()) < 1e-8 * float(mu_c.abs().max())


def test_restated_product_equals_the_dense_matrix():
    """``matvec`` (the product formulas, K never formed) against ``dense`` @ V, square with coincident points and rectangular."""
    gen = torch.Generator().manual_seed(12)
    for d, n, m in [(1, 6, 0), (3, 7, 5), (4, 5, 9)]:
        x1 = torch.rand(n, d, generator=gen, dtype=torch.float64)
        x2 = x1 if m == 0 else torch.rand(m, d, generator=gen, dtype=torch.float64)
        ls = 0.3 + 0.5 * torch.rand(d, generator=gen, dtype=torch.float64)
        V = torch.randn(x2.shape[0] * (d + 1), 3, generator=gen, dtype=torch.float64)
        assert float((R.matvec(x1, x2, ls, V) - R.dense(x1, x2, ls) @ V).abs().max()) < 1e-12
