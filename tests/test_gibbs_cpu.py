"""GibbsKernel without a device: the oracle and the dense branch against the fixture made by executing the reference's own code
(tests/golden/make_gibbs_golden.py), the rule of the native form, the constructor surface, the family row, the prepared rows and their torch
restatement, the chain rule of the hyper-gradient assembly, and the C ABI's refusals."""
import os
import re

import numpy as np
import pytest
import torch

from tests.gibbs_ref import MLP, field, gibbs_diag, gibbs_grad_sums, gibbs_K, prefactor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gibbs_values.npz")
CASES = [f"d{d}{s}{p}" for d in (1, 2, 3, 6) for s in "et" for p in ("64", "32")]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _case(gold, name):
    return {k: torch.from_numpy(gold[f"{name}_{k}"]) for k in ("x1", "x2", "K", "diag_same", "diag_pair")}


class Field(torch.nn.Module):
    def forward(self, x):
        return field(x)


def _fixture_f32_level(gold):
    """The rounding level the fixture itself shows: the largest distance of a float32 case of the reference from the float64 closed form."""
    worst = 0.0
    for name in CASES:
        if name.endswith("32"):
            c = _case(gold, name)
            ref = gibbs_K(c["x1"], field(c["x1"].double()), c["x2"], field(c["x2"].double()))
            worst = max(worst, float((c["K"].double() - ref).abs().max()))
    return worst


def test_fixture_covers_the_cases(gold):
    assert sorted({k.split("_")[0] for k in gold.files}) == sorted(CASES)
    for name in CASES:
        c = _case(gold, name)
        dt = torch.float64 if name.endswith("64") else torch.float32
        n, m = c["x1"].shape[0], c["x2"].shape[0]
        assert 12 <= n <= 17 and c["x1"].dtype == dt and c["K"].dtype == dt and c["K"].shape == (n, m)
        assert c["x1"].shape[1] == int(name[1]) and (("e" in name) == bool(c["x1"].shape == c["x2"].shape and torch.equal(c["x1"], c["x2"])))
        assert c["diag_same"].shape == (n,) and c["diag_pair"].shape == (min(n, m),)


@pytest.mark.parametrize("name", CASES)
def test_oracle_and_dense_branch_match_the_reference(gold, name):
    from gpytorch_amd import kernels as K
    from gpytorch_amd.operators import DenseLinearOperator, to_dense

    c = _case(gold, name)
    x1, x2 = c["x1"], c["x2"]
    f64 = name.endswith("64")
    k = min(x1.shape[0], x2.shape[0])
    # float64: 1e-12.  float32: the fixture's own distance from the float64 closed form -- the reference's rounding, 1.05e-6 over the eight float32
    # cases: its Gram-form squared distance carries about eps |x|^2 of absolute error, which the division by l^2 + l'^2 >= 0.013 magnifies -- times 4
    # for two float32 evaluations that round independently.  The sanity window only says that the fixture is float32-rounded and not worse.
    level = _fixture_f32_level(gold)
    assert 1e-8 < level < 1e-5
    tol = 1e-12 if f64 else 4.0 * level
    l1, l2 = field(x1.double()), field(x2.double())
    assert float((gibbs_K(x1, l1, x2, l2) - c["K"].double()).abs().max()) < (1e-12 if f64 else 2.0 * level)
    assert float((gibbs_diag(x1[:k], l1[:k], x2[:k], l2[:k]) - c["diag_pair"].double()).abs().max()) < (1e-12 if f64 else 2.0 * level)
    assert float((c["diag_same"].double() - 1.0).abs().max()) < (1e-15 if f64 else 1e-6)
    dense = K.gibbs_dense(Field(), x1, x2)
    assert dense.dtype == x1.dtype and float((dense.double() - c["K"].double()).abs().max()) < tol
    assert float((K.gibbs_dense(Field(), x1, x1, diag=True).double() - c["diag_same"].double()).abs().max()) < tol
    assert float((K.gibbs_dense(Field(), x1[:k], x2[:k], diag=True).double() - c["diag_pair"].double()).abs().max()) < tol
    if f64:   # the kernel object on the CPU in float64 takes the dense branch and returns the same values
        ker = K.GibbsKernel(Field())
        op = ker(x1, x2)
        assert isinstance(op, DenseLinearOperator) and float((to_dense(op) - c["K"]).abs().max()) < 1e-12
        assert float((ker(x1[:k], x2[:k], diag=True) - c["diag_pair"]).abs().max()) < 1e-12


def test_dense_is_torch_equal_for_identical_inputs_and_differentiable():
    from gpytorch_amd import kernels as K

    x = torch.rand(9, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(K.gibbs_dense(Field(), x, x), K.gibbs_dense(Field(), x, x.clone()))
    assert torch.equal(K.gibbs_dense(Field(), x, x).diagonal(), torch.ones(9, dtype=torch.float64))
    fn = MLP(d=2, dtype=torch.float64)
    xb = torch.rand(3, 7, 2, dtype=torch.float64)
    out = K.gibbs_dense(fn, xb, xb[:, :5])
    assert out.shape == (3, 7, 5)
    ref = torch.stack([gibbs_K(xb[b], fn(xb[b]), xb[b, :5], fn(xb[b, :5])) for b in range(3)])
    assert float((out.detach() - ref.detach()).abs().max()) < 1e-12
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fn.parameters())


def test_gibbs_native_truth_table():
    from gpytorch_amd import kernels as K

    ker = K.GibbsKernel(MLP(d=3))
    x, y = torch.rand(10, 3), torch.rand(7, 3)
    assert K.gibbs_native(ker, x) and K.gibbs_native(ker, x, y) and K.gibbs_native(ker, x, x)
    assert K.gibbs_native(K.GibbsKernel(Field()), torch.rand(10, 1)) and K.gibbs_native(K.GibbsKernel(Field()), torch.rand(10, 6))
    assert not K.gibbs_native(K.GibbsKernel(Field()), torch.rand(10, 7))                       # d > 6
    assert not K.gibbs_native(ker, x.double()) and not K.gibbs_native(ker, x, y.double())       # float64 inputs
    assert not K.gibbs_native(K.GibbsKernel(MLP(d=3, dtype=torch.float64)), x)                  # a float64 lengthscale_fn
    assert not K.gibbs_native(ker, x.expand(2, 10, 3)) and not K.gibbs_native(ker, x, y.expand(2, 7, 3))   # batches of inputs
    assert not K.gibbs_native(K.GibbsKernel(MLP(d=3), batch_shape=torch.Size([2])), x)           # a batch shape on the kernel
    assert not K.gibbs_native(ker, x, last_dim_is_batch=True)
    assert not K.gibbs_native(ker, x.clone().requires_grad_(True)) and not K.gibbs_native(ker, x, y.clone().requires_grad_(True))
    assert not K.gibbs_native(ker, x, torch.rand(7, 2))
    # pure: a meta tensor has shapes and dtypes and no device memory at all
    assert K.gibbs_native(ker, torch.empty(10, 3, device="meta"))


def test_constructor_surface():
    from gpytorch_amd import kernels as K

    with pytest.raises(NotImplementedError, match="does not support ARD"):
        K.GibbsKernel(Field(), ard_num_dims=2)
    ker = K.GibbsKernel(MLP())
    assert ker.is_stationary is False and ker.has_lengthscale is False and ker.lengthscale is None
    assert [n for n, _ in ker.named_parameters()] == ["lengthscale_fn.w1", "lengthscale_fn.b1", "lengthscale_fn.w2", "lengthscale_fn.b2"]
    assert ker[0] is ker
    kb = K.GibbsKernel(Field(), batch_shape=torch.Size([3, 2]))
    assert kb.batch_shape == torch.Size([3, 2])
    assert kb[1].batch_shape == torch.Size([2]) and kb[:, 0].batch_shape == torch.Size([3]) and kb[1:, :].batch_shape == torch.Size([2, 2])
    assert kb.batch_shape == torch.Size([3, 2]) and kb[1] is not kb

    class Bad(torch.nn.Module):
        def forward(self, x):
            return torch.ones(*x.shape[:-1], 2, dtype=x.dtype)

    with pytest.raises(ValueError, match=re.escape("lengthscale_fn must return shape (..., k, 1), got (..., k, 2)")):
        K.GibbsKernel(Bad())(torch.rand(5, 1))
    with pytest.raises(ValueError, match="lengthscale_fn must return shape"):
        K.gibbs_dense(Bad(), torch.rand(5, 1), torch.rand(4, 1))
    # active_dims select the columns lengthscale_fn sees
    x = torch.rand(6, 3, dtype=torch.float64)
    from gpytorch_amd.operators import to_dense

    ka = K.GibbsKernel(Field(), active_dims=[0, 2])
    assert float((to_dense(ka(x)) - gibbs_K(x[:, [0, 2]], field(x[:, [0, 2]]))).abs().max()) < 1e-12


def test_family_row():
    from gpytorch_amd import backend as B
    from gpytorch_amd import families as F

    assert F.KIND_IDS["gibbs"] == 10 and sorted(F.KIND_IDS.values()) == list(range(11))
    fam = F.FAMILIES["gibbs"]
    assert fam.id == 10 and fam.plan_kind == "gibbs"
    assert fam.one_kernel is True and fam.has_f64 is False and fam.widenable is False and fam.stackable is False
    assert fam.cov is F.gibbs_cov and fam.launch is not None and fam.grad_param is None
    assert isinstance(fam.coef, str) and "no preparation factor" in fam.coef
    assert F.GIBBS_PREFACTOR_EXPONENT == 0.5 and B.GIBBS_MAX_DIM == 6
    assert [F.gibbs_width(d) for d in range(1, 7)] == [4, 4, 8, 8, 8, 8]
    with pytest.raises(ValueError, match="float32 only"):
        fam.prepare(torch.rand(5, 3, dtype=torch.float64), None, None)
    with pytest.raises(ValueError, match="no batches"):
        fam.prepare(torch.rand(2, 5, 3), None, None)
    with pytest.raises(ValueError, match="1 <= d <= 6"):
        fam.prepare(torch.rand(5, 8), None, None)
    with pytest.raises(ValueError, match="1 <= d <= 6"):
        fam.prepare(torch.rand(5, 1), None, None)


def _prepared(x, l, shift=None):
    from gpytorch_amd import backend as B
    from gpytorch_amd import families as F

    z = torch.cat([x, l.reshape(-1, 1)], -1).float()
    par, lead, rows = F.FAMILIES["gibbs"].prepare(z, shift, None)
    assert lead is None
    return B.PreparedPoints(rows, z.shape[0], par.width, rows.shape[1], "gibbs", par)


@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_prepared_rows_and_gibbs_cov(d):
    from gpytorch_amd import families as F

    g = torch.Generator().manual_seed(40 + d)
    x1, x2 = torch.rand(23, d, generator=g, dtype=torch.float64), torch.rand(17, d, generator=g, dtype=torch.float64)
    l1 = 0.05 * d + 0.25 * d * torch.rand(23, generator=g, dtype=torch.float64)
    l2 = 0.05 * d + 0.25 * d * torch.rand(17, generator=g, dtype=torch.float64)
    shift = torch.cat([x1.mean(0), torch.zeros(1, dtype=torch.float64)]).float()
    p1, p2 = _prepared(x1, l1, shift), _prepared(x2, l2, shift)
    w = 4 if d <= 2 else 8
    assert p1.xp.shape == (23, w) and p1.xp.dtype == torch.float32 and p1.d == w and p1.dp == w and p1.param.d == d and p1.fused
    l32 = l1.float().double()   # the cloud is float32: the rows are exact functions of the ROUNDED l and x
    assert torch.equal(p1.xp[:, 0], (l32 * l32).float())
    assert float((p1.xp[:, 1].double() - 2.0 ** 0.25 * l32.sqrt()).abs().max()) < 1e-7   # (one float32 rounding of a value below 1.1)
    assert torch.equal(p1.xp[:, 2 : 2 + d], (x1.float().double() - shift[:d].double()).float())
    assert torch.equal(p1.xp[:, 2 + d :], torch.zeros(23, w - 2 - d))
    ref = gibbs_K(x1.float(), l1.float(), x2.float(), l2.float())
    assert float((F.gibbs_cov(p1, p2).double() - ref).abs().max()) < 1e-6
    rows = torch.tensor([5, 0, 22, 5])
    assert float((F.gibbs_cov(p1, p2, rows=rows).double() - ref[rows]).abs().max()) < 1e-6
    pd = _prepared(x1[:17], l1[:17], shift)
    assert float((F.gibbs_cov(pd, p2, diag=True).double() - gibbs_diag(x1[:17].float(), l1[:17].float(), x2.float(), l2.float())).abs().max()) < 1e-6
    assert torch.equal(F.gibbs_cov(p1, p1, diag=True), torch.ones(23))
    assert float((F.gibbs_cov(p1, p1).diagonal() - 1.0).abs().max()) < 5e-7
    # the prefactor alone: coincident points
    pre = F.gibbs_cov(_prepared(x1[:1].expand(23, d), l1, shift), _prepared(x1[:1].expand(17, d), l2, shift))
    assert float((pre.double() - prefactor(l1.float(), l2.float())).abs().max()) < 1e-6
    # a non-positive lengthscale gives NaN, as in the reference; nothing raises
    bad = _prepared(x1, torch.cat([-l1[:1], l1[1:]]), shift)
    k = F.gibbs_cov(bad, p2)
    assert torch.isnan(k[0]).all() and torch.isfinite(k[1:]).all()


@pytest.mark.parametrize("d,same,scaled", [(1, False, True), (3, True, True), (6, False, False), (2, True, False)])
def test_hyper_grads_from_sums_equal_autograd(d, same, scaled):
    """The assembly of ``functions._gibbs_hyper_grads`` from the derivative kernel's sums, those sums computed here from the closed form
    dk/dl_i = k (1/(2 l_i) - l_i u^2 + 2 s l_i u^4): against float64 autograd through an MLP lengthscale_fn, every parameter, at 1e-10."""
    from gpytorch_amd import functions as Fn

    g = torch.Generator().manual_seed(70 + d)
    n, m = 19, (19 if same else 14)
    x1 = torch.rand(n, d, generator=g, dtype=torch.float64)
    x2 = x1 if same else torch.rand(m, d, generator=g, dtype=torch.float64)
    fn = MLP(d=d, seed=3, dtype=torch.float64)
    W = torch.randn(n, m, generator=g, dtype=torch.float64)
    os_ = torch.tensor([1.7], dtype=torch.float64, requires_grad=True) if scaled else None

    # float64 autograd of the whole thing
    l1 = fn(x1)
    l2 = l1 if same else fn(x2)
    from tests.gibbs_ref import gibbs_k

    obj = (W * gibbs_k(x1, l1, x2, l2)).sum() * (os_.reshape(()) if scaled else 1.0)
    params = list(fn.parameters()) + ([os_] if scaled else [])
    want = torch.autograd.grad(obj, params)

    # the sums, from the closed form of the header
    with torch.no_grad():
        a, b = l1.reshape(-1, 1), l2.reshape(1, -1)
        s = (x1.unsqueeze(1) - x2.unsqueeze(0)).square().sum(-1)
        u2 = 1.0 / (a * a + b * b)
        k = gibbs_k(x1, l1, x2, l2)
        g0 = (W * k).sum()
        g1 = (W * k * (0.5 / a - a * u2 + 2.0 * s * a * u2 * u2)).sum(1)
        g2 = (W * k * (0.5 / b - b * u2 + 2.0 * s * b * u2 * u2)).sum(0)
    r0, r1, r2 = gibbs_grad_sums(x1, l1, x2, l2, W)
    assert float((g1 - r1).abs().max()) < 1e-10 * float(r1.abs().max()) and float((g2 - r2).abs().max()) < 1e-10 * float(r2.abs().max())

    # the operator's points are z = [x.detach() | l]; the Functions hand d_x1 / d_x2 to autograd, which carries their last column into fn
    z1 = torch.cat([x1.detach(), fn(x1)], -1)
    z2 = z1 if same else torch.cat([x2.detach(), fn(x2)], -1)
    p1 = _prepared(x1, l1.detach())
    p2 = p1 if same else _prepared(x2, l2.detach())
    ones = torch.ones(1, 1, dtype=torch.float64)
    out = Fn._gibbs_hyper_grads(p1, p2, ones, None if os_ is None else os_.detach(), None, None, (True, True), None, sums=(g0, g1, g2))
    d_ls, d_os, d_z1, d_z2 = out
    assert torch.equal(d_ls, torch.zeros(1, 1, dtype=torch.float64))
    assert d_z1.shape == (n, d + 1) and d_z2.shape == (m, d + 1)
    assert torch.equal(d_z1[:, :d], torch.zeros(n, d, dtype=torch.float64)) and torch.equal(d_z2[:, :d], torch.zeros(m, d, dtype=torch.float64))
    if same:
        got = torch.autograd.grad(z1, list(fn.parameters()), grad_outputs=d_z1 + d_z2)
    else:
        got = torch.autograd.grad([z1, z2], list(fn.parameters()), grad_outputs=[d_z1, d_z2])
    for gw, gg in zip(want, got):
        assert float((gw - gg).abs().max()) < 1e-10 * max(1.0, float(gw.abs().max()))
    if scaled:
        assert abs(float(d_os) - float(want[-1])) < 1e-10 * max(1.0, abs(float(want[-1])))
    else:
        assert d_os is None
    # one flag at a time, and none
    o1 = Fn._gibbs_hyper_grads(p1, p2, ones, None, None, None, (True, False), None, sums=(g0, g1, g2))
    assert o1[3] is None and torch.equal(o1[2][:, -1], g1)
    o2 = Fn._gibbs_hyper_grads(p1, p2, ones, None, None, None, (False, True), None, sums=(g0, g1, g2))
    assert o2[2] is None and torch.equal(o2[3][:, -1], g2)
    assert len(Fn._gibbs_hyper_grads(p1, p2, ones, None, None, None, (False, False), None, sums=(g0, g1, g2))) == 2
    with pytest.raises(RuntimeError, match="no learnable-parameter slot"):
        Fn._gibbs_hyper_grads(p1, p2, ones, None, None, None, (True, True), ones, sums=(g0, g1, g2))


def test_own_hyper_grads_dispatch_keeps_the_single_flag_for_the_other_families(monkeypatch):
    """``hyper_grads`` hands the Gibbs function (want_x1, want_x2) and the spectral-mixture / Newton-Girard functions the single flag they took before."""
    from gpytorch_amd import functions as Fn

    seen = {}

    def spy(name):
        def f(xp1, xp2, ls, os_, lt, rt, want_x, kparam, **kw):
            seen[name] = want_x
            return ()
        return f

    for name in ("sm", "ng", "gibbs"):
        monkeypatch.setitem(Fn._OWN_HYPER_GRADS, name, spy(name))

    class XP:
        def __init__(self, name):
            from gpytorch_amd import families as F

            self.family, self.dtype = F.FAMILIES[name], torch.float32

    for name in ("sm", "ng", "gibbs"):
        Fn.hyper_grads(XP(name), XP(name), None, None, None, None, want_x1=True, want_x2=False)
    assert seen == {"sm": True, "ng": True, "gibbs": (True, False)}
    for name in ("sm", "ng", "gibbs"):
        Fn.hyper_grads(XP(name), XP(name), None, None, None, None)
    assert seen == {"sm": False, "ng": False, "gibbs": (False, False)}


def _err(h):
    return h.gpamd_last_error()


def test_header_exports_and_abi_version():
    import subprocess

    from gpytorch_amd._lib import LIB_PATH, SIGNATURES, lib

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpamd.h")).read()
    assert re.search(r"GPAMD_GIBBS\s*=\s*10\b", header) and "#define GPAMD_ABI_VERSION 5" in header
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-nm") else "nm"
    out = subprocess.run([nm, "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ("gpamd_kv_gibbs_grad_f32", "gpamd_kv_gibbs_grad_workspace_doubles"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in exported and name in SIGNATURES and hasattr(h, name)
    for text in ("l_i^2 | 2^(1/4) sqrt(l_i)", "width 4 (d <= 2) or 8 (d <= 6)", "1/2 for EVERY d", "GIBBS_PREFACTOR_EXPONENT"):
        assert text in header, text


def test_abi_refusals_before_any_launch():
    """Every refusal of the new kind and the new entry points, with null buffers throughout: nothing can have been launched."""
    import ctypes as C

    from gpytorch_amd._lib import lib

    h = lib()
    GIBBS, SPLIT = 10, 8
    raw = C.create_string_buffer(256)
    p = C.addressof(raw)                                            # a non-null host address: not dereferenced by a refused call
    # the plan: the prepared width is 4 or 8; GPAMD_KV_SPLIT is required
    S, jc, ws = C.c_int(), C.c_int(), C.c_int64()
    for w in (4, 8):
        assert h.gpamd_kv_plan(GIBBS, 2000, 3000, w, 11, SPLIT, 2000, C.byref(S), C.byref(jc), C.byref(ws)) == 0
        assert S.value >= 1 and jc.value % 128 == 0 and S.value * jc.value >= 3000 and ws.value > S.value * 11 * 2000
    for w in (1, 2, 3, 5, 6, 7, 12):
        assert h.gpamd_kv_plan(GIBBS, 2000, 2000, w, 11, SPLIT, 2000, None, None, None) == -1
        assert _err(h).startswith(b"kv_plan: the Gibbs family takes d = the prepared width 4")
        assert h.gpamd_kv_partials_f32(GIBBS, 0.0, None, 300, None, 300, w, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1
        assert _err(h).startswith(b"kv: the Gibbs family takes d = the prepared width 4")
    for flags in (0, 1):
        assert h.gpamd_kv_plan(GIBBS, 2000, 2000, 4, 11, flags, 2000, None, None, None) == -1 and b"GPAMD_KV_SPLIT" in _err(h)
        assert h.gpamd_kv_partials_f32(GIBBS, 0.0, None, 300, None, 300, 4, None, None, 300, 11, None, 300, 1, 384, flags, None, None) == -1
        assert _err(h).startswith(b"kv: the Gibbs family") and b"GPAMD_KV_SPLIT" in _err(h)
    rc = h.gpamd_kv_partials_far_f32(GIBBS, 0.0, None, 300, None, 300, 4, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None, None, None, None, None,
                                     4.0, None, 0)
    assert rc == -1 and b"the Gibbs family is not culled" in _err(h)
    # a valid call gets as far as the shape checks
    assert h.gpamd_kv_partials_f32(GIBBS, 0.0, None, 300, None, 300, 8, None, None, 302, 11, None, 300, 1, 384, SPLIT, None, None) == -1
    assert b"leading dimensions" in _err(h)
    assert h.gpamd_kv_partials_f32(GIBBS, 0.0, None, 300, None, 300, 8, None, None, 300, 0, None, 300, 1, 384, SPLIT, None, None) == -1
    # every other entry point that takes a kind refuses the family
    assert h.gpamd_prep_points_f32(GIBBS, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_f32(GIBBS, 0.0, None, 300, None, 300, 4, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
    assert h.gpamd_kernel_dense_f32(GIBBS, 0.0, None, 10, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_rows_f32(GIBBS, 0.0, None, None, 3, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_diag_f32(GIBBS, 0.0, None, None, 10, 4, None, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_grad_f32(GIBBS, None, 300, None, 300, 4, None, 300, None, 300, 9, 0, None, None, 0, None) == -1
    for kind in (11, 31, 32):                                       # kinds beyond the new one stay unknown
        assert h.gpamd_kv_plan(kind, 2000, 2000, 4, 11, SPLIT, 2000, None, None, None) == -1
        assert h.gpamd_kv_partials_f32(kind, 0.0, None, 300, None, 300, 4, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1 and b"unknown kind" in _err(h)
    # the derivative entry point: width, null pointers, counts, leading dimensions, workspace
    ok = dict(X1p=p, n=300, X2p=p, m=200, width=4, Lt=p, ldl=300, Rt=p, ldr=200, t=9, out=p, ws=p, nws=1 << 40, st=None)

    def call(**kw):
        a = dict(ok, **kw)
        return h.gpamd_kv_gibbs_grad_f32(*[a[k] for k in ("X1p", "n", "X2p", "m", "width", "Lt", "ldl", "Rt", "ldr", "t", "out", "ws", "nws", "st")])

    for w in (0, 2, 6, 12, 16):
        assert call(width=w) == -2 and _err(h).startswith(b"kv_gibbs_grad: the prepared width must be 4")
        assert h.gpamd_kv_gibbs_grad_workspace_doubles(300, 200, 9, w) == 0
    for name in ("X1p", "X2p", "Lt", "Rt", "out", "ws"):
        assert call(**{name: None}) == -1 and _err(h).startswith(b"kv_gibbs_grad: bad arguments"), name
    for kw in (dict(n=0), dict(m=0), dict(t=0), dict(t=-3), dict(ldl=299), dict(ldr=199)):
        assert call(**kw) == -1 and _err(h).startswith(b"kv_gibbs_grad: bad arguments"), kw
    for w in (4, 8):
        need = h.gpamd_kv_gibbs_grad_workspace_doubles(300, 200, 9, w)
        assert need >= 300 + 3                                      # one slab of row sums and one sum per row block, at least
        assert call(width=w, nws=need - 1) == -3 and b"workspace smaller than gpamd_kv_gibbs_grad_workspace_doubles" in _err(h)
    assert h.gpamd_kv_gibbs_grad_workspace_doubles(0, 200, 9, 4) == 0 and h.gpamd_kv_gibbs_grad_workspace_doubles(300, 200, 0, 4) == 0
    # more than one column group doubles the workspace
    assert h.gpamd_kv_gibbs_grad_workspace_doubles(300, 200, 129, 4) == 2 * h.gpamd_kv_gibbs_grad_workspace_doubles(300, 200, 128, 4)


def test_python_plans_under_its_own_kind():
    from gpytorch_amd import backend as B

    for n, m, t in [(2000, 2000, 11), (100_000, 100_000, 65), (257, 300, 140), (2000, 2000, 33), (2000, 2000, 34)]:
        ld = B.round_up(n, 4)
        for w in (4, 8):
            S, jc, ws = B.kv_plan("gibbs", n, m, w, t, B.KV_SPLIT, ld)
            assert S >= 1 and jc % 128 == 0 and S * jc >= m and (S - 1) * jc < m
            groups = max(1, (t - 1 + 31) // 32)   # 32 columns per launch group, a trailing 33rd rides as the extra column
            assert ws >= S * t * ld + 32 * groups * B.round_up(m, 128)   # the f16 planes of V: one 32-row pair per column group
