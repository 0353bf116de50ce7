"""CPU: the product-structure kernel (``kernels.ProductStructureKernel``, the native family ``"ps"`` = tensor-product Matern) -- the float64
restatement and ``ps_dense`` against the reference's own outputs (tests/golden/product_structure_values.npz, made by
tests/golden/make_product_structure_golden.py), the rule ``ps_native``, the routing of ``forward``, the s^d rule, the ABI's refusals with null
buffers (nothing launches) and the torch restatement ``families.ps_cov`` on prepared rows."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

import gpytorch_amd as g
from gpytorch_amd import backend as B
from gpytorch_amd import operators
from gpytorch_amd.kernels import (GridInterpolationKernel, MaternKernel, ProductStructureKernel, RBFKernel, RQKernel, ScaleKernel, ps_dense, ps_native)
from tests.product_structure_ref import FAMILIES, MATERN, ps_cov, ps_terms
from tests.test_ski_cpu import _Fake

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_structure_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files if k.endswith("_x1")})
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def _case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


def _tol(dt):
    return 1e-12 if dt == np.float64 else 4e-6     # (tests/test_additive_cpu.py's bounds for its float64 / float32 golden cases)


def _abs_err(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def _base(kind, **kw):
    return RBFKernel(**kw) if kind == "rbf" else MaternKernel(nu=NU[kind], **kw)


def _psk(base, d, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return ProductStructureKernel(base, num_dims=d, **kw)


def test_fixture_covers_the_cases():
    dims = {GOLD[f"{c}_x1"].shape[1] for c in CASES}
    assert dims == {2, 3, 6, 8, 9} and all(GOLD[f"{c}_x1"].shape[0] <= 31 and GOLD[f"{c}_x2"].shape[0] <= 31 for c in CASES)
    assert {GOLD[f"{c}_x1"].dtype for c in CASES} == {np.dtype("float32"), np.dtype("float64")}
    assert {bool(GOLD[f"{c}_same"]) for c in CASES} == {True, False} and {GOLD[f"{c}_ls"].shape[1] == 1 for c in CASES} == {True, False}


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name, kind):
    """The float64 closed form (tests/product_structure_ref.py) against the reference's own outputs: 1e-12 in the float64 cases, 4e-6 in the float32
    cases, absolute; with the inner outputscale s the values carry s^d and so does the bound.  (The closed form differs from the reference by the
    rounding of the reference's distance; on this fixture that stays below the bounds -- the float32 two-input case has at most 25 points per cloud,
    where ``torch.cdist`` takes differences and not the quadratic expansion.)"""
    c = _case(name)
    x1, x2, ls = (torch.as_tensor(c[k]) for k in ("x1", "x2", "ls"))
    d = x1.shape[1]
    tol = _tol(c["x1"].dtype)
    k = min(x1.shape[0], x2.shape[0])
    sd = float(c["os"]) ** d
    K = ps_cov(kind, x1, x2, ls)
    errs = (_abs_err(K, c[f"K_{kind}"]), _abs_err(sd * K, c[f"Ks_{kind}"]) / max(1.0, sd),
            _abs_err(sd * ps_cov(kind, x1, x1, ls, diag=True), c[f"diag_same_{kind}"]) / max(1.0, sd),
            _abs_err(sd * ps_cov(kind, x1[:k], x2[:k], ls, diag=True), c[f"diag_pair_{kind}"]) / max(1.0, sd))
    print("restatement", name, kind, errs)
    assert max(errs) < tol, errs
    assert K.dtype == torch.float64 and torch.equal(ps_terms(kind, x1, x2, ls).prod(-1), K) and ps_terms(kind, x1, x2, ls).shape == (*K.shape, d)


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("name", CASES)
def test_ps_dense_matches_the_reference(name, kind):
    """``kernels.ps_dense`` against the reference's own outputs: 1e-12 in float64, 4e-6 in float32, absolute -- K without and with the inner
    ScaleKernel (s^d), ``diag=True`` of one input and of two; in the dtype of the inputs; a batch of two copies gives two copies."""
    c = _case(name)
    dt = torch.float64 if c["x1"].dtype == np.float64 else torch.float32
    x1, x2 = torch.as_tensor(c["x1"]), torch.as_tensor(c["x2"])
    if bool(c["same"]):
        x2 = x1
    d = x1.shape[1]
    tol = _tol(c["x1"].dtype)
    base = _base(kind, ard_num_dims=d if c["ls"].shape[1] > 1 else None).to(dt)
    base.lengthscale = torch.as_tensor(c["ls"])
    sk = ScaleKernel(base).to(dt)
    sk.outputscale = torch.as_tensor(c["os"])
    k = min(x1.shape[0], x2.shape[0])
    with torch.no_grad():
        K, Ks = ps_dense(base, x1, x2), ps_dense(sk, x1, x2)
        errs = [_abs_err(K, c[f"K_{kind}"]), _abs_err(Ks, c[f"Ks_{kind}"]), _abs_err(ps_dense(sk, x1, x1, diag=True), c[f"diag_same_{kind}"]),
                _abs_err(ps_dense(sk, x1[:k], x2[:k], diag=True), c[f"diag_pair_{kind}"])]
        print(name, kind, errs)
        assert K.dtype == dt and max(errs) < tol * max(1.0, float(c["os"]) ** d), errs
        Kb = ps_dense(sk, x1.expand(2, *x1.shape), x2.expand(2, *x2.shape))
        assert Kb.shape == (2, *K.shape) and _abs_err(Kb[1], Ks) < tol * max(1.0, float(c["os"]) ** d)


def test_ps_native_envelope():
    def kern(d=3, base=None, inner=False, num_dims=None, ard=True):
        b = MaternKernel(nu=2.5, ard_num_dims=d if ard else None) if base is None else base
        return _psk(ScaleKernel(b) if inner else b, d if num_dims is None else num_dims)

    x = _Fake((10, 3))
    assert ps_native(kern(), x) and ps_native(kern(inner=True), x, _Fake((7, 3))) and ps_native(kern(ard=False), x)
    assert ps_native(kern(), _Fake((10, 3), device="cpu"))                               # pure: never looks at the device
    for nu in (0.5, 1.5, 2.5):
        assert ps_native(kern(base=MaternKernel(nu=nu)), x)
    # float32 parameters and inputs
    assert not ps_native(kern(), _Fake((10, 3), dtype=torch.float64)) and not ps_native(kern(), x, _Fake((7, 3), dtype=torch.float64))
    assert not ps_native(kern().double(), x) and not ps_native(kern(inner=True).double(), x)
    # no batch shapes, no last_dim_is_batch
    assert not ps_native(kern(), _Fake((2, 10, 3))) and not ps_native(kern(), x, _Fake((2, 7, 3))) and not ps_native(kern(), x, last_dim_is_batch=True)
    assert not ps_native(kern(base=MaternKernel(nu=2.5, batch_shape=torch.Size([2]))), x)
    batched = kern(inner=True)
    batched.base_kernel = ScaleKernel(MaternKernel(nu=2.5), batch_shape=torch.Size([2]))
    assert not ps_native(batched, x)
    # 2 <= d <= 8 and d == num_dims
    assert ps_native(kern(d=2), _Fake((10, 2))) and ps_native(kern(d=8), _Fake((10, 8)))
    assert not ps_native(kern(d=1), _Fake((10, 1))) and not ps_native(kern(d=9), _Fake((10, 9)))
    assert not ps_native(kern(num_dims=4, ard=False), x) and not ps_native(kern(), x, _Fake((7, 2)))
    # the base exactly a MaternKernel, bare or inside ONE unbatched ScaleKernel
    assert not ps_native(kern(base=RBFKernel()), x) and not ps_native(kern(base=RQKernel()), x)
    assert not ps_native(kern(base=ScaleKernel(ScaleKernel(MaternKernel(nu=1.5)))), x)
    assert not ps_native(kern(base=MaternKernel(nu=1.5, active_dims=[0])), x)
    assert not ps_native(kern(base=MaternKernel(nu=1.5) + MaternKernel(nu=2.5)), x)
    # a lengthscale shaped [1, 1] or [1, d]
    assert not ps_native(kern(base=MaternKernel(nu=1.5, ard_num_dims=2)), x)
    # inputs without requires_grad
    assert not ps_native(kern(), _Fake((10, 3), requires_grad=True)) and not ps_native(kern(), x, _Fake((7, 3), requires_grad=True))


def test_forward_routing_scale_rule_diag_and_errors():
    gen = torch.Generator().manual_seed(3)
    x, x2 = torch.rand(15, 4, generator=gen), torch.rand(9, 4, generator=gen)
    ls = 0.5 + 0.4 * torch.rand(1, 4, generator=gen)
    # the deprecation warning and the last_dim_is_batch error are the reference's
    with pytest.warns(DeprecationWarning, match="ProductStructureKernel is deprecated, and will be removed in GPyTorch 2.0"):
        ProductStructureKernel(MaternKernel(nu=2.5), num_dims=4)
    kern = _psk(ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=4)), 4)
    kern.base_kernel.base_kernel.lengthscale, kern.base_kernel.outputscale = ls, 1.3
    with pytest.raises(RuntimeError, match="ProductStructureKernel does not accept the last_dim_is_batch argument."):
        kern(x, last_dim_is_batch=True)
    assert kern.is_stationary and kern.num_outputs_per_input(x, x) == 1 and _psk(RBFKernel(), 3, active_dims=[0, 2, 3]).active_dims.tolist() == [0, 2, 3]
    assert kern.prediction_strategy is kern.base_kernel.prediction_strategy
    # Matern base: ONE fused operator of kind "ps", code = the base family's id, lengthscale [1, d], outputscale s^d (differentiable); nothing launches
    for single in (False, True):
        base = MaternKernel(nu=1.5, ard_num_dims=None if single else 4)
        k2 = _psk(ScaleKernel(base), 4)
        base.lengthscale, k2.base_kernel.outputscale = (0.7 if single else ls), 1.3
        for a, b in ((x, None), (x, x2)):
            op = k2(a) if b is None else k2(a, b)
            assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "ps" and op.spec.code == 2 and op.spec.param is None
            assert op.shape == (15, 15 if b is None else 9) and tuple(op.lengthscale.shape) == (1, 4)
            assert abs(float(op.outputscale.detach()) - 1.3 ** 4) < 1e-5 and op.outputscale.requires_grad
        (gr,) = torch.autograd.grad(op.outputscale.sum(), [k2.base_kernel.raw_outputscale])
        assert abs(float(gr) - 4 * 1.3 ** 3 * (1 - math.exp(-1.3))) < 1e-4            # d s^(d-1) ds/draw, softplus
        bare = _psk(base, 4)(x, x2)
        assert bare.spec.kind == "ps" and (bare.outputscale is None or abs(float(bare.outputscale) - 1.0) < 1e-6)
    # diag: the same input -> s^d ones (no launch); two different inputs -> dense elementwise products
    dg = kern(x, diag=True)
    assert dg.shape == (15,) and torch.allclose(dg.detach(), torch.full((15,), 1.3 ** 4)) and dg.requires_grad
    want = 1.3 ** 4 * ps_cov("matern52", x[:9], x2, ls, diag=True)
    assert _abs_err(kern(x[:9], x2, diag=True).detach(), want) < 4e-6
    # RBF base: the operator RBFKernel(ard_num_dims=d) returns -- kind "rbf", lengthscale [1, d], scale s^d
    for single in (False, True):
        rb = RBFKernel(ard_num_dims=None if single else 4)
        kr = _psk(ScaleKernel(rb), 4)
        rb.lengthscale, kr.base_kernel.outputscale = (0.7 if single else ls), 1.3
        op = kr(x, x2)
        assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "rbf" and tuple(op.lengthscale.shape) == (1, 4)
        assert abs(float(op.outputscale.detach()) - 1.3 ** 4) < 1e-5
        ard = RBFKernel(ard_num_dims=4)
        ard.lengthscale = rb.lengthscale.detach().expand(1, 4)
        twin, mine = ard(x, x2), _psk(rb, 4)(x, x2)
        assert type(twin) is type(mine) and twin.spec.kind == mine.spec.kind and torch.equal(twin.lengthscale, mine.lengthscale)
        assert torch.equal(twin.spec.shift, mine.spec.shift) and mine.outputscale is None
        assert torch.allclose(kr(x, diag=True).detach(), torch.full((15,), 1.3 ** 4))
    op9 = _psk(RBFKernel(), 9)(torch.rand(6, 9, generator=gen))
    assert isinstance(op9, operators.FusedKernelLinearOperator) and op9.spec.kind == "rbf"          # RBF: any d >= 2
    # d = 1: the base kernel itself
    k1 = _psk(MaternKernel(nu=2.5), 1)
    o1 = k1(x[:, :1])
    assert isinstance(o1, operators.FusedKernelLinearOperator) and o1.spec.kind == "matern52"
    # declined calls: DenseLinearOperator of ps_dense -- float64, d = 9 over Matern, inputs that require grad (other base kernels densify on the device)
    x64 = x.double()
    out = kern.double()(x64)
    assert isinstance(out, operators.DenseLinearOperator)
    l64 = kern.base_kernel.base_kernel.lengthscale.detach().reshape(-1)
    s64 = float(kern.base_kernel.outputscale.detach())
    assert _abs_err(operators.to_dense(out).detach(), s64 ** 4 * ps_cov("matern52", x64, x64, l64)) < 1e-12
    x9 = torch.rand(6, 9, generator=gen)
    assert isinstance(_psk(MaternKernel(nu=0.5), 9)(x9), operators.DenseLinearOperator)
    xg = x.clone().requires_grad_(True)
    og = _psk(MaternKernel(nu=2.5), 4)(xg)
    assert isinstance(og, operators.DenseLinearOperator)
    operators.to_dense(og).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    # a grid base on the host (float64 / the CPU): the dense product of the dimension batch, d of them
    gk = GridInterpolationKernel(RBFKernel(), grid_size=12, num_dims=1, grid_bounds=[(0.0, 1.0)]).double()
    kg = _psk(gk, 2)
    og = kg(x64[:, :2])
    assert isinstance(og, operators.DenseLinearOperator)
    assert _abs_err(operators.to_dense(og).detach(), gk.dimension_batch(x64[:, :2], x64[:, :2]).prod(-3).detach()) < 1e-14


def test_exports():
    for name in ("ProductStructureKernel", "ps_native", "ps_dense"):
        assert name in g.kernels.__all__ and hasattr(g.kernels, name)
    assert B.PS_KIND_ID == 11 and B.FAMILIES["ps"].id == 11 and B.ps_code("matern32") == 2
    with pytest.raises(ValueError, match="per-dimension lengthscales"):
        B.ps_code("rbf")


def test_family_traits():
    f = B.FAMILIES["ps"]
    assert f.id == 11 and f.name == "ps" and f.plan_kind == "add" and f.one_kernel and not f.has_f64 and not f.widenable and not f.stackable
    assert f.cov is B.ps_cov and f.launch is not None and f.grad_param is None
    from gpytorch_amd.functions import KernelSpec, _OWN_HYPER_GRADS

    assert KernelSpec("ps", code=3).param_value() == 3 and "ps" in _OWN_HYPER_GRADS
    x = torch.rand(5, 3)
    par, lead, rows = f.prepare(x, None, 2)
    assert (par.base, par.d, par.base_kind) == (2, 3, "matern32") and lead == (2, 0.0) and rows is None
    for bad in (0, 4, 1.5, None):
        with pytest.raises(ValueError):
            f.prepare(x, None, bad)
    with pytest.raises(ValueError):
        f.prepare(torch.rand(5, 9), None, 2)
    with pytest.raises(ValueError):
        f.prepare(x.double(), None, 2)
    with pytest.raises(ValueError):
        f.prepare(torch.rand(2, 5, 3), None, 2)


def _rows(x, ls, kind, d, shift=None):
    """Prepared rows of the BASE family built in torch: z = coef (x - shift) / l per column, stride round_up(d, 4), zero padding."""
    dp = B.round_up(d, 4)
    z = (x if shift is None else x - shift) / ls * B.prep_coef(kind)
    return B.PreparedPoints(torch.nn.functional.pad(z.float(), (0, dp - d)).contiguous(), x.shape[0], d, dp, "ps", B.PSParams(B.ps_code(kind), d))


@pytest.mark.parametrize("kind", MATERN)
def test_ps_cov_on_prepared_rows(kind):
    """``families.ps_cov`` (float32, the kernel's arithmetic: one exponential of the L1 sum, the polynomials, pairwise product) against the float64
    restatement on the float32 rows' own values: d factors of a few float32 ulp each and an exponent error <= eps sum r, k <= 1 -- 2e-6 absolute."""
    gen = torch.Generator().manual_seed(5)
    for d in (2, 3, 5, 8):
        x1, x2 = torch.rand(9, d, generator=gen).double(), torch.rand(7, d, generator=gen).double()
        ls = 0.5 + 0.4 * torch.rand(d, generator=gen).double()
        p1, p2 = _rows(x1, ls, kind, d), _rows(x2, ls, kind, d)
        assert p1.dp == (4 if d <= 4 else 8) and torch.equal(p1.xp[:, d:], torch.zeros(9, p1.dp - d))
        z1, z2 = p1.xp[:, :d].double() / B.prep_coef(kind), p2.xp[:, :d].double() / B.prep_coef(kind)
        want = ps_cov(kind, z1, z2, torch.ones(d))
        assert _abs_err(want, ps_cov(kind, x1, x2, ls)) < 1e-5
        assert _abs_err(B.ps_cov(p1, p2), want) < 2e-6 and B.ps_cov(p1, p2).dtype == torch.float32
        S = 1.7
        assert _abs_err(B.kernel_dense(p1, p2, torch.tensor([S])), S * want) < 2e-6 * S
        rows = torch.tensor([4, 0, 8])
        assert _abs_err(B.kernel_rows(p1, rows, p2), want[rows]) < 2e-6
        assert _abs_err(B.kernel_diag(_rows(x1[:7], ls, kind, d), p2), want[:7].diagonal()) < 2e-6
        assert torch.equal(B.kernel_diag(p1, p1), torch.ones(9)) and torch.equal(B.kernel_dense(p1, p1).diagonal(), torch.ones(9))     # exact ones
        assert B.prep_coef_of(p1) == B.prep_coef(kind)
        # policy: one kernel, never culled, no Gram-form derivative, no float64 fused path, planned as the additive family
        for t in (1, 5, 33, 65):
            assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        with g.settings.far_pair_cutoff(1e-3):
            assert B.far_cull(p1, p2) is None
        assert not B.grad_gram_ok(p1, p2) and not B.f64_widenable(p1)
        assert B.kv_plan("ps", 2000, 2000, d, 11, B.KV_SPLIT, 2000) == B.kv_plan("add", 2000, 2000, d, 11, B.KV_SPLIT, 2000)


def test_hyper_grads_from_sums():
    """``functions._ps_hyper_grads`` on sums handed in (nothing launches): d/dl_q = s sums[1 + q] (-2 / l_q), summed for one lengthscale; d/ds =
    sums[0]; input gradients and a learnable-parameter slot are refused, naming the family."""
    from gpytorch_amd.functions import _ps_hyper_grads, hyper_grads

    gen = torch.Generator().manual_seed(9)
    d, kind = 3, "matern52"
    x1, x2 = torch.rand(8, d, generator=gen).double(), torch.rand(6, d, generator=gen).double()
    W = torch.randn(8, 6, generator=gen).double()
    ls = (0.5 + 0.4 * torch.rand(d, generator=gen).double()).requires_grad_(True)
    s = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    terms = ps_terms(kind, x1, x2, ls)
    K = terms.prod(-1)
    g_ls, g_s = torch.autograd.grad((W * (s * K)).sum(), [ls, s])
    # the sums the derivative kernel is specified to return, from the closed forms of include/gpamd.h
    r = ((x1.unsqueeze(1) - x2.unsqueeze(0)) / ls.detach()).abs() * math.sqrt(5.0)
    rho = -r * r * (1 + r) / (6 * (1 + r + r * r / 3))
    sums = torch.cat([(W * K.detach()).sum().reshape(1), (W.unsqueeze(-1) * K.detach().unsqueeze(-1) * rho).sum((0, 1))])
    p = _rows(x1, ls.detach(), kind, d)
    d_ls, d_os = _ps_hyper_grads(p, p, ls.detach().reshape(1, d), s.detach().reshape(1), None, None, False, None, sums=sums)
    assert _abs_err(d_ls.reshape(-1), g_ls) < 1e-12 * float(g_ls.abs().max()) + 1e-13 and abs(float(d_os) - float(g_s)) < 1e-12
    one = torch.tensor([[0.7]], dtype=torch.float64)
    d1, _ = _ps_hyper_grads(p, p, one, None, None, None, False, None, sums=sums)
    assert d1.shape == (1, 1) and abs(float(d1) - float((-2.0 / 0.7 * sums[1:]).sum())) < 1e-12
    with pytest.raises(RuntimeError, match="'ps'"):
        hyper_grads(p, p, one, None, None, None, want_x1=True)
    with pytest.raises(RuntimeError, match="'ps'"):
        hyper_grads(p, p, one, None, None, None, want_x2=True)


def _err(h):
    return h.gpamd_last_error()


def test_abi_header_exports_and_refusals_before_any_launch():
    from gpytorch_amd._lib import SIGNATURES, lib

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpamd.h")).read()
    assert "GPAMD_PS = 11" in header and "GPAMD_ABI_VERSION 5" in header.replace("  ", " ")
    for name in ("gpamd_kv_ps_partials_f32", "gpamd_kv_ps_grad_workspace_doubles", "gpamd_kv_ps_grad_f32"):
        assert name in header and name in SIGNATURES and hasattr(h, name)
    tail = (None, 300, None, 300, None, 300, 11, None, 300, 1, 384, None, None)            # X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk, done, stream
    gtail = (None, 300, None, 300, None, 300, None, 300, 8, None, None, 0, None)           # X1p, n, X2p, m, Lt, ldl, Rt, ldr, t, out, ws, ws_doubles, stream
    for d in (1, 9, 0, 33, -2):
        assert h.gpamd_kv_ps_partials_f32(2, d, *tail) == -2 and _err(h).startswith(b"kv_ps:") and b"2..8" in _err(h)
        assert h.gpamd_kv_ps_grad_f32(2, d, *gtail) == -2 and _err(h).startswith(b"kv_ps_grad:") and b"2..8" in _err(h)
        assert h.gpamd_kv_ps_grad_workspace_doubles(300, 300, 8, d) == 0
    # base = 0: a product of one-dimensional RBFs IS the RBF family with per-dimension lengthscales
    assert h.gpamd_kv_ps_partials_f32(0, 4, *tail) == -1 and _err(h).startswith(b"kv_ps:") and b"RBF family with per-dimension lengthscales" in _err(h)
    assert h.gpamd_kv_ps_grad_f32(0, 4, *gtail) == -1 and _err(h).startswith(b"kv_ps_grad:") and b"RBF family with per-dimension lengthscales" in _err(h)
    for base in (-1, 4, 9):
        assert h.gpamd_kv_ps_partials_f32(base, 4, *tail) == -1 and _err(h).startswith(b"kv_ps:") and b"base family" in _err(h)
        assert h.gpamd_kv_ps_grad_f32(base, 4, *gtail) == -1 and _err(h).startswith(b"kv_ps_grad:") and b"base family" in _err(h)
    # a valid call gets as far as the shape checks of the shared launch code (what gpamd_kv_partials_f32 refuses) / the null-pointer check of the derivative
    for base in (1, 2, 3):
        bad_ldv = tail[:5] + (302,) + tail[6:]
        assert h.gpamd_kv_ps_partials_f32(base, 4, *bad_ldv) == -1 and b"leading dimensions" in _err(h)
        assert h.gpamd_kv_ps_partials_f32(base, 4, *(tail[:6] + (0,) + tail[7:])) == -1 and b"bad shape" in _err(h)
        assert h.gpamd_kv_ps_grad_f32(base, 4, *gtail) == -1 and _err(h).startswith(b"kv_ps_grad: bad arguments")
    # the derivative entry point: null pointers, counts, leading dimensions, workspace (a non-null address that is never read: every refusal is before a launch)
    import ctypes as C

    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    ok = [p, 300, p, 200, p, 300, p, 200, 9, p, p, 1 << 40, None]
    need = h.gpamd_kv_ps_grad_workspace_doubles(300, 200, 9, 4)
    assert need > 0 and need % 5 == 0
    for i in (0, 2, 4, 6, 9, 10):                                                           # each pointer null in turn
        a = list(ok)
        a[i] = None
        assert h.gpamd_kv_ps_grad_f32(3, 4, *a) == -1 and _err(h).startswith(b"kv_ps_grad: bad arguments")
    for i, v in ((1, 0), (3, 0), (8, 0), (5, 299), (7, 199)):                               # n, m, t, ldl, ldr
        a = list(ok)
        a[i] = v
        assert h.gpamd_kv_ps_grad_f32(3, 4, *a) == -1 and _err(h).startswith(b"kv_ps_grad: bad arguments")
    a = list(ok)
    a[11] = need - 1
    assert h.gpamd_kv_ps_grad_f32(3, 4, *a) == -3 and _err(h).startswith(b"kv_ps_grad:") and b"workspace" in _err(h)
    # the workspace query: 1 + d doubles per unit
    w = {d: h.gpamd_kv_ps_grad_workspace_doubles(300, 300, 8, d) for d in (2, 4, 8)}
    assert w[2] * 5 == w[4] * 3 and w[4] * 9 == w[8] * 5 and w[2] > 0
    # the plan is the additive family's; every entry point that takes a kind refuses 11 as the unknown kind it was
    PS, SPLIT = 11, 8
    assert h.gpamd_kv_plan(8, 2000, 2000, 4, 11, SPLIT, 2000, None, None, None) == 0
    assert h.gpamd_kv_plan(PS, 2000, 2000, 4, 11, SPLIT, 2000, None, None, None) == -1
    assert h.gpamd_kv_partials_f32(PS, 0.0, None, 300, None, 300, 4, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_prep_points_f32(PS, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_dense_f32(PS, 0.0, None, 10, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_rows_f32(PS, 0.0, None, None, 3, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_diag_f32(PS, 0.0, None, None, 10, 4, None, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_grad_f32(PS, None, 300, None, 300, 4, None, 300, None, 300, 9, 0, None, None, 0, None) == -1
    assert h.gpamd_kv_f32(PS, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
    assert h.gpamd_pivoted_cholesky_f32(PS, 0.0, None, 100, 4, None, 5, 1e-3, None, 100, None, None, None, None) == -1
