"""CPU: the Newton-Girard additive family (``GPAMD_NG`` = 9, ``kernels.NewtonGirardAdditiveKernel``) -- ``ng_dense`` against the reference's own outputs,
identities that involve no recursion, ``ng_native``'s rule, the gradient assembly ``functions._ng_hyper_grads``, the kernel's API and every refusal of the
C ABI before any launch.  Oracle of the values: tests/newton_girard_ref.py (float64 closed forms), fixture: tests/golden/newton_girard_values.npz."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from tests.newton_girard_ref import FAMILIES, add_terms, dim_dists, esp, ng_cov, ng_cov_normalised, ng_grad_sums, ng_norm

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "newton_girard_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def _case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


def _base(g, kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=NU[kind], **kw)


def _ng(base, d, r=None, **kw):
    import gpytorch_amd as g

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return g.kernels.NewtonGirardAdditiveKernel(base, num_dims=d, max_degree=r, **kw)


def _pin_lengthscale(base, ls):
    """``base.lengthscale`` is the fixture's tensor EXACTLY (set through the softplus constraint it comes back one ulp off in some cases, which the
    reference's Gram-trick distance amplifies): the arithmetic is what these tests pin, not the round trip through the constraint."""
    base.lengthscale = ls
    fixed = ls.clone().requires_grad_(True)
    base._get_transformed = lambda name: fixed
    return base


def _fixture_figure():
    """max over cases, families and the three outputs of |fixture - closed form| / k(x, x)."""
    worst = 0.0
    for name in CASES:
        c = _case(name)
        x1, x2 = c["x1"], c["x2"]
        k = min(x1.shape[0], x2.shape[0])
        s = float(ng_norm(c["sigma"], x1.shape[1]))
        for kind in FAMILIES:
            for key, a, b, dg in (("K", x1, x2, False), ("diag_same", x1, x1, True), ("diag_pair", x1[:k], x2[:k], True)):
                err = (ng_cov(kind, a, b, c["ls"], c["sigma"], diag=dg) - torch.from_numpy(c[f"{key}_{kind}"]).double()).abs().max()
                worst = max(worst, float(err) / s)
    return worst


_FIGURE = []


def _figure():
    if not _FIGURE:
        _FIGURE.append(_fixture_figure())
    return _FIGURE[0]


def test_fixture_covers_the_cases():
    seen = set()
    for name in CASES:
        c = _case(name)
        d, r = c["x1"].shape[1], c["sigma"].shape[0]
        same = c["x1"].shape == c["x2"].shape and np.array_equal(c["x1"], c["x2"])
        seen.add((d, r))
        seen.add(("combo", str(c["x1"].dtype), c["ls"].shape[-1] > 1, same))
        assert max(c["x1"].shape[0], c["x2"].shape[0]) <= 32 and c["ls"].shape in ((1, 1), (1, d))
        assert all(f"{key}_{kind}" in c for kind in FAMILIES for key in ("K", "diag_same", "diag_pair"))
    for d in (2, 3, 5, 8):
        for r in {1, 2, 3, d}:
            assert r > d or (d, r) in seen, (d, r)
    for dt in ("float64", "float32"):
        for ard in (False, True):
            for same in (False, True):
                assert ("combo", dt, ard, same) in seen, (dt, ard, same)


@pytest.mark.parametrize("name", CASES)
def test_ng_dense_matches_the_reference(name):
    """``kernels.ng_dense`` against the reference's own outputs, all cases, all four bases, K and both diagonals.  The tolerance does not come from the
    code under test: the reference allocates its polynomials in float32 whatever the inputs are and evaluates them by an alternating sum, so the
    fixture itself is off the float64 closed form (tests/newton_girard_ref.py).  Measured here, max over cases of |fixture - closed form| / k(x, x):
    3.7e-6 (the float32 cases; 1.0e-7 over the float64 cases alone).  ``ng_dense`` must be within 4 x that figure of the fixture, and the figure
    above 1e-5 fails outright.  (Measured: ``ng_dense`` is 1.0e-7 from the float64 fixtures -- it is 7.4e-15 from the closed form there -- and
    6.0e-7 from the float32 ones, whose distance arithmetic it shares.)"""
    import gpytorch_amd as g
    from gpytorch_amd.kernels import ng_dense

    fig = _figure()
    print("fixture vs closed form:", fig)
    assert fig <= 1e-5, fig
    c = _case(name)
    x1, x2, ls, sigma = (torch.from_numpy(c[key]) for key in ("x1", "x2", "ls", "sigma"))
    dt, d, r = x1.dtype, x1.shape[1], sigma.numel()
    s = float(ng_norm(sigma, d))
    k = min(x1.shape[0], x2.shape[0])
    for kind in FAMILIES:
        base = _pin_lengthscale(_base(g, kind, ard_num_dims=d if ls.shape[-1] > 1 else None).to(dt), ls)
        with torch.no_grad():
            K = ng_dense(base, x1, x2, sigma, r)
            outs = ((K, "K"), (ng_dense(base, x1, x1, sigma, r, diag=True), "diag_same"), (ng_dense(base, x1[:k], x2[:k], sigma, r, diag=True), "diag_pair"))
            errs = [float((o.double() - torch.from_numpy(c[f"{key}_{kind}"]).double()).abs().max()) / s for o, key in outs]
            print("ng_dense", name, kind, errs)
            assert K.dtype == dt and K.shape == (x1.shape[0], x2.shape[0]) and max(errs) <= 4 * fig, (kind, errs, fig)
            # any batch: leading batch dimensions on inputs and outputscales give the same matrices
            Kb = ng_dense(base, x1.expand(2, *x1.shape), x2.expand(2, *x2.shape), sigma.expand(2, r), r)
            assert Kb.shape == (2, *K.shape) and float((Kb[1] - K).abs().max()) / s <= 4 * fig
    # autograd-visible, finite gradients (coinciding points included: x1 against itself)
    sg = sigma.clone().requires_grad_(True)
    Kg = ng_dense(base, x1, x1, sg, r)
    gl, gs = torch.autograd.grad(Kg.sum(), [base.lengthscale, sg])
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gs).all())


def _f64_setup(kind, d, n=13, m=9, ard=True, seed=0):
    import gpytorch_amd as g

    gen = torch.Generator().manual_seed(100 + seed)
    x1, x2 = torch.rand(n, d, generator=gen, dtype=torch.float64), torch.rand(m, d, generator=gen, dtype=torch.float64)
    base = _base(g, kind, ard_num_dims=d if ard else None).double()
    base.lengthscale = 0.2 + 0.5 * torch.rand(1, d if ard else 1, generator=gen, dtype=torch.float64)
    return g, base, x1, x2


@pytest.mark.parametrize("kind", FAMILIES)
def test_identities_without_any_recursion(kind):
    """float64, 1e-12 of k(x, x): max_degree = 1 is ``additive_dense`` with sigma_1; a one-hot sigma at n = d over an RBF base is the ARD RBF kernel;
    sigma = 1 with max_degree = d is prod_q (1 + z_q) - 1."""
    from gpytorch_amd.kernels import additive_dense, ng_dense

    for d in (2, 3, 5, 8):
        g, base, x1, x2 = _f64_setup(kind, d, seed=d)
        with torch.no_grad():
            for a, b in ((x1, x2), (x1, x1)):
                s1 = torch.tensor([0.7], dtype=torch.float64)
                assert float((ng_dense(base, a, b, s1, 1) - 0.7 * additive_dense(base, a, b)).abs().max()) <= 1e-12 * 0.7 * d
                assert float((ng_dense(base, a, b, s1, 1, diag=True) - 0.7 * additive_dense(base, a, b[: a.shape[0]], diag=True)).abs().max()) <= 1e-12 * 0.7 * d \
                    if a.shape[0] == b.shape[0] else True
                ones = torch.ones(d, dtype=torch.float64)
                z = add_terms(kind, a, b, base.lengthscale.reshape(-1))
                want = (1 + z).prod(-1) - 1
                assert float((ng_dense(base, a, b, ones, d) - want).abs().max()) <= 1e-12 * (2 ** d - 1)
                if kind == "rbf":
                    hot = torch.zeros(d, dtype=torch.float64)
                    hot[d - 1] = 1.0
                    ard = torch.exp(-0.5 * dim_dists(a, b, base.lengthscale.reshape(-1)).square().sum(-1))    # the ARD RBFKernel, closed form
                    assert float((ng_dense(base, a, b, hot, d) - ard).abs().max()) <= 1e-12


def test_closed_form_oracle_is_self_consistent():
    """The oracle's subset enumeration against two facts it does not use: e_n of d ones is C(d, n), and sum_n e_n = prod (1 + z) - 1."""
    z = torch.rand(7, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    e = esp(z, 6)
    assert float((sum(e) - ((1 + z).prod(-1) - 1)).abs().max()) < 1e-13
    assert [float(v[0]) for v in esp(torch.ones(1, 8, dtype=torch.float64), 8)] == [float(math.comb(8, n)) for n in range(1, 9)]
    x = torch.rand(5, 4, dtype=torch.float64)
    assert torch.allclose(ng_cov_normalised("matern32", x, x, [0.3], [0.2, 0.5, 0.1], diag=True), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-14)


def test_ng_native_truth_table():
    import gpytorch_amd as g
    from gpytorch_amd.kernels import ng_native

    R, M, S = g.kernels.RBFKernel, g.kernels.MaternKernel, g.kernels.ScaleKernel
    x4, x9 = torch.rand(12, 4), torch.rand(12, 9)
    for d in range(2, 9):
        x = torch.rand(10, d)
        for r in (None, 1, 2, d):
            assert ng_native(_ng(R(), d, r), x)
            assert ng_native(_ng(R(ard_num_dims=d), d, r), x, torch.rand(7, d))
            for nu in (0.5, 1.5, 2.5):
                assert ng_native(_ng(M(nu=nu, ard_num_dims=d), d, r), x)
                assert ng_native(_ng(M(nu=nu), d, r), x)
    yes = _ng(R(ard_num_dims=4), 4, 3)
    assert ng_native(yes, x4) and ng_native(yes, x4, None) and ng_native(yes, x4, x4)
    no = [
        ("float64 inputs", _ng(R(), 4), x4.double(), None, {}),
        ("float64 model", _ng(R(), 4).double(), x4, None, {}),
        ("float64 base only", _ng(R().double(), 4), x4, None, {}),
        ("float64 x2", _ng(R(), 4), x4, x4.double(), {}),
        ("input batch", _ng(R(), 4), torch.rand(2, 12, 4), None, {}),
        ("x2 batch", _ng(R(), 4), x4, torch.rand(2, 12, 4), {}),
        ("kernel batch", _ng(R(), 4, batch_shape=torch.Size([2])), x4, None, {}),
        ("base batch", _ng(R(batch_shape=torch.Size([2])), 4), x4, None, {}),
        ("d = 9", _ng(R(), 9), x9, None, {}),
        ("d = 1", _ng(R(), 1), torch.rand(12, 1), None, {}),
        ("d != num_dims", _ng(R(), 5), x4, None, {}),
        ("x2 of another d", _ng(R(), 4), x4, torch.rand(5, 3), {}),
        ("rq base", _ng(g.kernels.RQKernel(), 4), x4, None, {}),
        ("periodic base", _ng(g.kernels.PeriodicKernel(), 4), x4, None, {}),
        ("pp base", _ng(g.kernels.PiecewisePolynomialKernel(), 4), x4, None, {}),
        ("ScaleKernel base", _ng(S(R()), 4), x4, None, {}),
        ("ScaleKernel Matern base", _ng(S(M(nu=2.5, ard_num_dims=4)), 4), x4, None, {}),
        ("base with active_dims", _ng(R(active_dims=[0]), 4), x4, None, {}),
        ("lengthscale of another width", _ng(R(ard_num_dims=3), 4), x4, None, {}),
        ("last_dim_is_batch", _ng(R(), 4), x4, None, {"last_dim_is_batch": True}),
        ("inputs that require grad", _ng(R(), 4), x4.clone().requires_grad_(True), None, {}),
        ("x2 that requires grad", _ng(R(), 4), x4, x4.clone().requires_grad_(True), {}),
    ]
    for name, kern, a, b, kw in no:
        assert ng_native(kern, a, b, **kw) is False, name
    assert ng_native(yes, x4) is True   # pure: a host call of the rule never touches a device


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("d,r,ard", [(3, 3, True), (4, 2, False), (5, 4, True), (8, 3, False), (2, 1, True)])
def test_hyper_grads_from_dense_sums_equal_autograd(kind, d, r, ard):
    """``functions._ng_hyper_grads`` fed with the sums computed densely in float64, routed through the kernel's own autograd graph (S in the
    outputscale slot, sigma in the parameter slot, the expanded lengthscale), against autograd through ``ng_dense``: raw lengthscale (single and
    ARD) and raw outputscale, 1e-10 relative to the largest gradient entry."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import _ng_hyper_grads
    from gpytorch_amd.kernels import ng_dense

    g, base, x1, x2 = _f64_setup(kind, d, n=11, m=8, ard=ard, seed=10 * d + r)
    kern = _ng(base, d, r).double()
    kern.outputscale = 0.2 + torch.rand(r, dtype=torch.float64, generator=torch.Generator().manual_seed(d))
    W = torch.randn(11, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(r))
    # autograd through the dense restatement
    want = torch.autograd.grad((W * ng_dense(base, x1, x2, kern.outputscale, r)).sum(), [base.raw_lengthscale, kern.raw_outputscale])
    # the native route, without a device: the three differentiable slots of the operator and the assembled gradients pushed back through them
    sigma = kern.outputscale
    scale = (sigma * B.ng_binomials(d, r, dtype=sigma.dtype)).sum().reshape(1)
    ls = base.lengthscale.expand(1, d)
    par = B.NGParams(B.add_code(base.kind), sigma, d)
    sums = ng_grad_sums(kind, x1, x2, ls.detach().reshape(-1), sigma.detach(), W, B.ng_cap(d, r))

    class _XP:
        param = par

    d_ls, d_os, d_sigma = _ng_hyper_grads(_XP, _XP, ls, scale, None, None, False, sigma, sums=sums)
    assert d_ls.shape == ls.shape and d_os.shape == scale.shape and d_sigma.shape == sigma.shape
    got = torch.autograd.grad([ls, scale, sigma], [base.raw_lengthscale, kern.raw_outputscale], [d_ls, d_os, d_sigma])
    for a, b, what in zip(got, want, ("raw_lengthscale", "raw_outputscale")):
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(kind, d, r, what, err)
        assert a.shape == b.shape and err < 1e-10, (what, err)
    # an outer scale multiplies the outputscale slot: every gradient scales with it, the normaliser S stays the family's own
    d_ls2, d_os2, d_sigma2 = _ng_hyper_grads(_XP, _XP, ls, 3.0 * scale, None, None, False, sigma, sums=sums)
    assert torch.allclose(d_ls2, 3.0 * d_ls, rtol=1e-13, atol=0) and torch.allclose(d_sigma2, 3.0 * d_sigma, rtol=1e-13, atol=0) and torch.equal(d_os2, d_os)
    with pytest.raises(RuntimeError, match="inputs are not provided"):
        _ng_hyper_grads(_XP, _XP, ls, scale, None, None, True, sigma, sums=sums)


def test_constructor_api_and_state_dict():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd import operators
    from gpytorch_amd.kernels import NewtonGirardAdditiveKernel, ng_dense, ng_native

    assert all(n in g.kernels.__all__ for n in ("NewtonGirardAdditiveKernel", "ng_native", "ng_dense"))
    assert ng_dense is g.kernels.ng_dense and ng_native is g.kernels.ng_native
    with pytest.warns(DeprecationWarning, match="NewtonGirardAdditiveKernel is deprecated"):
        kern = NewtonGirardAdditiveKernel(g.kernels.RBFKernel(ard_num_dims=4), num_dims=4, max_degree=3)
    assert kern.num_dims == 4 and kern.max_degree == 3 and kern.is_stationary and kern.active_dims is None
    assert kern.raw_outputscale.shape == (3,) and torch.allclose(kern.outputscale, torch.full((3,), 1 / 3))
    assert _ng(g.kernels.RBFKernel(), 4).max_degree == 4 and _ng(g.kernels.RBFKernel(), 4, 9).max_degree == 4    # None: d; above d: capped silently
    assert _ng(g.kernels.RBFKernel(), 4, 9).raw_outputscale.shape == (4,)
    assert _ng(g.kernels.RBFKernel(), 3, 2, batch_shape=torch.Size([5])).raw_outputscale.shape == (5, 2)
    assert _ng(g.kernels.RBFKernel(), 3, active_dims=[0, 2, 3]).active_dims.tolist() == [0, 2, 3]
    kern.outputscale = [0.5, 0.25, 2.0]
    assert torch.allclose(kern.outputscale, torch.tensor([0.5, 0.25, 2.0])) and bool((kern.raw_outputscale != 0).all())
    kern.outputscale = torch.tensor([0.1, 0.2, 0.3])
    assert torch.allclose(kern.outputscale, torch.tensor([0.1, 0.2, 0.3]))
    x = torch.rand(15, 4)
    with pytest.raises(RuntimeError, match="does not accept the last_dim_is_batch argument"):
        kern(x, last_dim_is_batch=True)
    # state-dict round trip
    other = _ng(g.kernels.RBFKernel(ard_num_dims=4), 4, 3)
    kern.base_kernel.lengthscale = torch.tensor([[0.2, 0.25, 0.3, 0.35]])
    other.load_state_dict(kern.state_dict())
    assert torch.equal(other.raw_outputscale, kern.raw_outputscale) and torch.equal(other.base_kernel.raw_lengthscale, kern.base_kernel.raw_lengthscale)
    assert set(kern.state_dict()) >= {"raw_outputscale", "base_kernel.raw_lengthscale"}
    # the native operator (built without a device): kind, code, sigma in the parameter slot, S in the scale slot, the expanded lengthscale
    for kind in FAMILIES:
        for ard in (False, True):
            base = _base(g, kind, ard_num_dims=4 if ard else None)
            base.lengthscale = torch.tensor([[0.2, 0.25, 0.3, 0.35]]) if ard else 0.3
            k3 = _ng(base, 4, 3)
            k3.outputscale = [0.5, 0.25, 2.0]
            op = k3(x)
            S = 0.5 * 4 + 0.25 * 6 + 2.0 * 4
            assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "ng" and op.spec.code == B.KIND_IDS[kind]
            assert op.spec.param.shape == (3,) and op.spec.param.requires_grad and op.requires_grad
            code, sig = op.spec.param_value()
            assert code == op.spec.code and not sig.requires_grad and torch.allclose(sig, torch.tensor([0.5, 0.25, 2.0]))
            assert op.x1 is op.x2 and op.shape == (15, 15) and op.lengthscale.shape == (1, 4) and op.lengthscale.requires_grad
            assert abs(float(op.outputscale.detach()) - S) < 1e-5 and op.outputscale.requires_grad
            assert torch.allclose(op.spec.shift, x.mean(0))
            (gl,) = torch.autograd.grad(op.lengthscale.sum(), base.raw_lengthscale)
            assert gl.shape == base.raw_lengthscale.shape
            assert k3(x, torch.rand(9, 4)).shape == (15, 9)
            dg = k3(x, diag=True)     # diag of one input: S, no launch
            assert dg.shape == (15,) and torch.allclose(dg, torch.full((15,), S)) and dg.requires_grad
            x2 = torch.rand(15, 4)    # diag of two different inputs: the dense branch
            want = ng_cov(kind, x, x2, base.lengthscale.detach().reshape(-1), [0.5, 0.25, 2.0], diag=True)
            assert float((k3(x, x2, diag=True).detach().double() - want).abs().max()) < 4e-6 * S
            outer = g.kernels.ScaleKernel(k3)   # an outer ScaleKernel multiplies into the scale slot
            outer.outputscale = 0.5
            oo = outer(x)
            assert isinstance(oo, operators.FusedKernelLinearOperator) and oo.spec.kind == "ng" and abs(float(oo.outputscale.detach()) - 0.5 * S) < 1e-5
    # declined calls: a DenseLinearOperator of ng_dense -- a ScaleKernel base (its outputscale enters e_n as s^n), float64
    inner = g.kernels.ScaleKernel(g.kernels.RBFKernel())
    inner.outputscale = 1.7
    ks = _ng(inner, 4, 2)
    out = ks(x)
    assert isinstance(out, operators.DenseLinearOperator)
    ls = inner.base_kernel.lengthscale.detach().double().reshape(-1)
    z = 1.7 * add_terms("rbf", x, x, ls)
    e = esp(z, 2)
    assert float((operators.to_dense(out).detach().double() - 0.5 * (e[0] + e[1])).abs().max()) < 4e-6 * 0.5 * (1.7 * 4 + 1.7 ** 2 * 6)
    x64 = x.double()
    k64 = _ng(g.kernels.RBFKernel().double(), 4, 3).double()
    k64.outputscale = torch.full((3,), 1 / 3, dtype=torch.float64)   # (a list goes through the default dtype, as in the reference)
    out = k64(x64)
    assert isinstance(out, operators.DenseLinearOperator)
    assert float((operators.to_dense(out).detach() - ng_cov("rbf", x64, x64, [0.6931471805599453], [1 / 3] * 3)).abs().max()) < 1e-12 * 14 / 3


def test_backend_parameters_and_policy():
    from gpytorch_amd import backend as B
    import gpytorch_amd as g

    assert B.KIND_IDS["ng"] == 9
    assert [B.ng_cap(d, r) for d, r in ((2, 1), (2, 2), (3, 3), (4, 1), (4, 3), (4, 4), (8, 3), (8, 4), (8, 8))] == [2, 2, 3, 3, 3, 4, 3, 8, 8]
    sig = torch.tensor([0.5, 0.25])
    par = B.NGParams(2, sig, 5)
    S = 0.5 * 5 + 0.25 * 10
    assert (par.base, par.base_kind, par.d, par.r, par.rc) == (2, "matern32", 5, 2, 3) and abs(float(par.s) - S) < 1e-12
    assert par.block.dtype == torch.float32 and torch.equal(par.block, torch.tensor([0.5 / S * 4096, 0.25 / S * 4096, 0.0]))
    for bad_base in (4, -1, 1.5):
        with pytest.raises(ValueError):
            B.NGParams(bad_base, sig, 5)
    with pytest.raises(ValueError, match="max_degree in 1..d"):
        B.NGParams(0, torch.ones(4), 3)
    with pytest.raises(ValueError):
        B.NGParams(0, sig, 9)
    # ng_esp: the recursion in the input dtype against the enumeration
    z = torch.rand(6, 5, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    for a, b in zip(B.ng_esp(z, 8), esp(z, 8)):
        assert float((a - b).abs().max()) < 1e-13 * float(b.max())
    assert B.ng_esp(z.float(), 3)[2].dtype == torch.float32
    # ng_cov on CPU-built prepared clouds against the closed form: rows, dense, diag (prepared coordinates carry the family constant)
    x1, x2 = torch.rand(9, 5), torch.rand(7, 5)
    ls = torch.tensor([0.3, 0.4, 0.5, 0.35, 0.45])
    for kind in FAMILIES:
        coef = B.prep_coef(kind)
        p = B.NGParams(B.add_code(kind), sig, 5)
        mk = lambda x: B.PreparedPoints(torch.nn.functional.pad(x / ls * coef, (0, 3)), x.shape[0], 5, 8, "ng", p)  # noqa: E731
        p1, p2 = mk(x1), mk(x2)
        want = ng_cov_normalised(kind, x1, x2, ls, sig)
        assert float((B.ng_cov(p1, p2).double() - want).abs().max()) < 2e-6
        assert float((B.kernel_dense(p1, p2, torch.tensor([S])).double() - S * want).abs().max()) < 2e-6 * S
        rows = torch.tensor([4, 0, 8])
        assert float((B.kernel_rows(p1, rows, p2).double() - want[rows]).abs().max()) < 2e-6
        assert float((B.kernel_diag(p1, p1).double() - 1.0).abs().max()) < 1e-6
        assert B.prep_coef_of(p1) == coef
        # policy: one kernel, never culled, no Gram-form derivative, no float64 fused path
        for t in (1, 5, 33, 65):
            assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        with g.settings.far_pair_cutoff(1e-3):
            assert B.far_cull(p1, p2) is None
        assert not B.grad_gram_ok(p1, p2) and not B.f64_widenable(p1)
    p64 = B.PreparedPoints(p1.xp.double(), 9, 5, 8, "ng", p)
    assert not B.fused_f64(p64, p64)


def _err(h):
    return h.gpamd_last_error()


def test_abi_refusals_before_any_launch():
    from gpytorch_amd._lib import lib
    import ctypes as C

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    blk = (C.c_float * 8)(*([1.0] * 8))
    blk = C.cast(blk, C.c_void_p)
    tail = (None, 300, None, 300, None, 300, 11, None, 300, 1, 384, None, None)            # X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk, done, stream
    gtail = (None, 300, None, 300, None, 300, None, 300, 8, None, None, 0, None)           # X1p, n, X2p, m, Lt, ldl, Rt, ldr, t, out, ws, ws_doubles, stream
    for d in (1, 9, 0, 33):
        assert h.gpamd_kv_ng_partials_f32(blk, 0, d, 1, *tail) == -2 and _err(h).startswith(b"kv_ng:") and b"2..8" in _err(h)
        assert h.gpamd_kv_ng_grad_f32(blk, 0, d, 1, *gtail) == -2 and _err(h).startswith(b"kv_ng_grad:") and b"2..8" in _err(h)
        assert h.gpamd_kv_ng_grad_workspace_doubles(300, 300, 8, d, 1) == 0
    assert h.gpamd_kv_ng_partials_f32(None, 0, 4, 2, *tail) == -1 and b"null weight block" in _err(h)
    assert h.gpamd_kv_ng_grad_f32(None, 0, 4, 2, *gtail) == -1 and b"null weight block" in _err(h)
    for base in (-1, 4, 9):
        assert h.gpamd_kv_ng_partials_f32(blk, base, 4, 2, *tail) == -1 and b"base family" in _err(h)
        assert h.gpamd_kv_ng_grad_f32(blk, base, 4, 2, *gtail) == -1 and b"base family" in _err(h)
    for d, r in ((4, 0), (4, 5), (2, 3), (8, 9), (8, -1)):
        assert h.gpamd_kv_ng_partials_f32(blk, 3, d, r, *tail) == -1 and b"max_degree" in _err(h)
        assert h.gpamd_kv_ng_grad_f32(blk, 3, d, r, *gtail) == -1 and b"max_degree" in _err(h)
        assert h.gpamd_kv_ng_grad_workspace_doubles(300, 300, 8, d, r) == 0
    # a valid call gets as far as the shape checks of the shared launch code (ldv % 4) / the null-pointer and workspace checks of the derivative
    bad_ldv = tail[:5] + (302,) + tail[6:]
    assert h.gpamd_kv_ng_partials_f32(blk, 3, 4, 2, *bad_ldv) == -1 and b"leading dimensions" in _err(h)
    assert h.gpamd_kv_ng_grad_f32(blk, 3, 4, 2, *gtail) == -1 and _err(h).startswith(b"kv_ng_grad: bad arguments")
    # the workspace query follows the degree cap: 1 + d + rc doubles per unit
    w = {(d, r): h.gpamd_kv_ng_grad_workspace_doubles(300, 300, 8, d, r) for d, r in ((8, 1), (8, 3), (8, 4), (8, 8), (4, 3), (4, 4))}
    assert w[8, 1] == w[8, 3] and w[8, 4] == w[8, 8] and w[8, 3] * 17 == w[8, 8] * 12 and w[4, 3] * 9 == w[4, 4] * 8 and w[8, 1] > 0
    # the plan is the additive family's; every entry point that takes a kind refuses 9
    NG, SPLIT = 9, 8
    assert h.gpamd_kv_plan(8, 2000, 2000, 4, 11, SPLIT, 2000, None, None, None) == 0
    assert h.gpamd_kv_plan(NG, 2000, 2000, 4, 11, SPLIT, 2000, None, None, None) == -1
    assert h.gpamd_prep_points_f32(NG, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_partials_f32(NG, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_f32(NG, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
    assert h.gpamd_kernel_dense_f32(NG, 0.0, None, 10, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_rows_f32(NG, 0.0, None, None, 3, None, 10, 4, None, None, 12, None) == -1
    assert h.gpamd_kernel_diag_f32(NG, 0.0, None, None, 10, 4, None, None, None) == -1
    assert h.gpamd_pivoted_cholesky_f32(NG, 0.0, None, 100, 4, None, 5, 1e-3, None, 100, None, None, None, None) == -1
    gargs = (None, 1000, None, 1000, 4, None, 1000, None, 1000, 8, 0, None, None, 0, None, None, None, None, None, 0.0, None, 0)
    assert h.gpamd_kv_grad_param_far_f32(NG, 0.0, *gargs) == -1 and h.gpamd_kv_grad_f32(NG, *gargs[:15]) == -1
    assert h.gpamd_prep_points_f64(NG, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1
    assert h.gpamd_kv_partials_f64(NG, 0.0, None, 300, None, 300, 4, None, 300, 11, None, 300, 1, 384, None, None) == -1


def test_python_plans_as_the_additive_family():
    from gpytorch_amd import backend as B

    for n, m, t, d in [(2000, 2000, 11, 4), (100_000, 100_000, 65, 8), (257, 300, 140, 2)]:
        ld = B.round_up(n, 4)
        assert B.kv_plan("ng", n, m, d, t, B.KV_SPLIT, ld) == B.kv_plan("add", n, m, d, t, B.KV_SPLIT, ld)
