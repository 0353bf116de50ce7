"""CPU: the additive family (``KIND_ADD`` / ``GPAMD_ADD`` = 8, ``kernels.AdditiveStructureKernel``) -- the restatement and ``additive_dense`` against the
reference's own outputs, ``additive_native``'s rule, the kernel's API, the code rule and every refusal of the C ABI before any launch.
Oracle of the values: tests/additive_ref.py, pinned to tests/golden/additive_values.npz."""
import os
import warnings

import numpy as np
import pytest
import torch

import math

from tests.additive_ref import FAMILIES, add_cov, add_mean, add_terms, dim_dists, ref_add_cov

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "additive_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def _case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


def _tol(dt):
    return 1e-12 if dt == np.float64 else 4e-6


def _base(g, kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=NU[kind], **kw)


def _asq(base, d, **kw):
    import gpytorch_amd as g

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return g.kernels.AdditiveStructureKernel(base, num_dims=d, **kw)


def test_fixture_covers_both_lengthscale_shapes_and_dtypes():
    shapes = {(_case(c)["ls"].shape[-1] == 1, _case(c)["x1"].dtype) for c in CASES}
    assert shapes == {(True, np.dtype("float64")), (False, np.dtype("float64")), (True, np.dtype("float32")), (False, np.dtype("float32"))}
    assert all(max(_case(c)["x1"].shape[0], _case(c)["x2"].shape[0]) <= 40 for c in CASES)


def _pin_lengthscale(base, ls):
    """Make ``base.lengthscale`` the fixture's tensor EXACTLY: set through the softplus constraint it comes back one ulp off in some ARD cases, and
    the reference's Gram-trick distance turns that ulp into 7e-6 of a float32 Matern-1/2 entry -- the arithmetic is what these tests pin, not the
    round trip through the constraint."""
    base.lengthscale = ls
    fixed = ls.clone().requires_grad_(True)
    base._get_transformed = lambda name: fixed
    return base


def _abs_err(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", FAMILIES)
def test_restatement_matches_the_reference(name, kind):
    """``ref_add_cov`` (the reference's executed arithmetic, restated over oracle/kernels.py) against the reference's own outputs: 1e-12 in float64,
    4e-6 in float32, absolute, on K and both diagonals.  The closed form the device tests use as their oracle differs from the reference by the
    ROUNDING OF THE REFERENCE'S DISTANCE (measured on these fixtures, worst family Matern-1/2: 2.5e-12 in float64 case b, 4.3e-13 in e; 9.1e-6 and
    2.4e-5 in the float32 cases f and g; <= 3e-15 / 1e-6 for the other families), so it is held to a bound worked out from the inputs: the expanded
    squared distance is off by delta <= 8 x 2^-53 (max |z1|^2 + max |z2|^2), a distance rho by delta / (2 rho), and no base family is steeper than
    sqrt(5) per unit of rho -- d sqrt(5) delta / (2 min rho) over the non-zero per-dimension distances, float64 cases only."""
    c = _case(name)
    tol = _tol(c["x1"].dtype)
    k = min(c["x1"].shape[0], c["x2"].shape[0])
    d = c["x1"].shape[1]
    errs = (_abs_err(ref_add_cov(kind, c["x1"], c["x2"], c["ls"]), c[f"K_{kind}"]),
            _abs_err(ref_add_cov(kind, c["x1"], c["x1"], c["ls"], diag=True), c[f"diag_same_{kind}"]),
            _abs_err(ref_add_cov(kind, c["x1"][:k], c["x2"][:k], c["ls"], diag=True), c[f"diag_pair_{kind}"]))
    print("restatement", name, kind, errs)
    assert max(errs) < tol, errs
    assert ref_add_cov(kind, c["x1"], c["x2"], c["ls"]).dtype == torch.from_numpy(c["x1"]).dtype
    if c["x1"].dtype == np.float64:
        x1, x2, ls = (torch.from_numpy(c[key]) for key in ("x1", "x2", "ls"))
        mean = x1.mean(0, keepdim=True)
        delta = 8 * 2.0 ** -53 * float(((x1 - mean) / ls).pow(2).max() + ((x2 - mean) / ls).pow(2).max())
        rho = dim_dists(x1, x2, ls)
        bound = d * math.sqrt(5.0) * delta / (2 * float(rho[rho > 0].min())) + 1e-14
        e_closed = _abs_err(add_cov(kind, x1, x2, ls), c[f"K_{kind}"])
        print("closed form", name, kind, e_closed, "bound", bound)
        assert e_closed < bound < 1e-8, (e_closed, bound)
        assert _abs_err(add_cov(kind, x1, x1, ls, diag=True), c[f"diag_same_{kind}"]) == 0.0
    assert torch.allclose(add_mean(kind, c["x1"], c["x2"], c["ls"]) * d, add_cov(kind, c["x1"], c["x2"], c["ls"]), rtol=0, atol=1e-14 * d)
    assert add_terms(kind, c["x1"], c["x2"], c["ls"]).shape == (c["x1"].shape[0], c["x2"].shape[0], d)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", FAMILIES)
def test_additive_dense_matches_the_reference(name, kind):
    """``kernels.additive_dense`` against the reference's own outputs: 1e-12 in float64, 4e-6 in float32, absolute -- K, ``diag=True`` of one input and
    of two, both lengthscale shapes (the fixture's cases).  Under a ScaleKernel it is the same matrix times the outputscale, exactly."""
    import gpytorch_amd as g
    from gpytorch_amd.kernels import additive_dense

    c = _case(name)
    dt = torch.from_numpy(c["x1"]).dtype
    x1, x2 = torch.from_numpy(c["x1"]), torch.from_numpy(c["x2"])
    d = x1.shape[1]
    ard = c["ls"].shape[-1] > 1
    base = _pin_lengthscale(_base(g, kind, ard_num_dims=d if ard else None).to(dt), torch.from_numpy(c["ls"]))
    tol = _tol(c["x1"].dtype)
    k = min(x1.shape[0], x2.shape[0])
    with torch.no_grad():
        K = additive_dense(base, x1, x2)
        errs = (_abs_err(K, c[f"K_{kind}"]), _abs_err(additive_dense(base, x1, x1, diag=True), c[f"diag_same_{kind}"]),
                _abs_err(additive_dense(base, x1[:k], x2[:k], diag=True), c[f"diag_pair_{kind}"]))
        print("additive_dense", name, kind, errs)
        assert K.dtype == dt and max(errs) < tol, errs
        # any batch: a leading batch dimension on the inputs gives the same matrices
        Kb = additive_dense(base, x1.expand(2, *x1.shape), x2.expand(2, *x2.shape))
        assert Kb.shape == (2, *K.shape) and _abs_err(Kb[1], K) < tol
        scaled = g.kernels.ScaleKernel(base).to(dt)
        scaled.outputscale = float(c["os"])
        assert torch.equal(additive_dense(scaled, x1, x2), K * scaled.outputscale)
        assert torch.equal(additive_dense(scaled, x1[:k], x2[:k], diag=True), additive_dense(base, x1[:k], x2[:k], diag=True) * scaled.outputscale)
    # autograd-visible, finite gradients (coinciding points included: x1 against itself)
    Kg = additive_dense(base, x1, x1)
    assert Kg.requires_grad
    (gl,) = torch.autograd.grad(Kg.sum(), base.lengthscale)
    assert bool(torch.isfinite(gl).all())


def test_float64_kernel_call_takes_the_dense_branch_and_matches():
    """The kernel's own call on float64 inputs (any device): a DenseLinearOperator holding ``additive_dense`` -- the reference's outputs to 1e-12,
    d = 9 and d = 8 alike; the diagonal of one input is d."""
    import gpytorch_amd as g
    from gpytorch_amd import operators

    for name in CASES:
        c = _case(name)
        if c["x1"].dtype != np.float64:
            continue
        x1, x2 = torch.from_numpy(c["x1"]), torch.from_numpy(c["x2"])
        d = x1.shape[1]
        ard = c["ls"].shape[-1] > 1
        for kind in FAMILIES:
            base = _pin_lengthscale(_base(g, kind, ard_num_dims=d if ard else None).double(), torch.from_numpy(c["ls"]))
            kern = _asq(base, d).double()
            out = kern(x1, x2)
            assert isinstance(out, operators.DenseLinearOperator)
            assert _abs_err(operators.to_dense(out).detach(), c[f"K_{kind}"]) < 1e-12
            assert _abs_err(kern(x1, diag=True).detach(), torch.full((x1.shape[0],), float(d), dtype=torch.float64)) < 1e-12
            assert isinstance(g.kernels.ScaleKernel(kern).double()(x1, x2), operators.DenseLinearOperator)


def test_multitask_dense_branch_knows_the_additive_kind():
    """``KroneckerFusedAddedDiagLinearOperator.to_dense_differentiable`` (the small-n Cholesky branch of a multitask model, torch ops only) with an
    additive data kernel: kron(d s k~, K_TT) + task noise, against the closed form (float32 parameters: 4e-6 of the largest entry)."""
    import gpytorch_amd as g
    from gpytorch_amd.multitask import KroneckerFusedAddedDiagLinearOperator, KroneckerFusedLinearOperator

    x = torch.rand(14, 3, generator=torch.Generator().manual_seed(4))
    ktt = torch.tensor([[1.5, 0.4], [0.4, 0.8]])
    noise = torch.tensor([0.1, 0.2])
    for kind in FAMILIES:
        inner = g.kernels.ScaleKernel(_base(g, kind, ard_num_dims=3))
        inner.base_kernel.lengthscale, inner.outputscale = torch.tensor([[0.2, 0.3, 0.35]]), 1.7
        kx = _asq(inner, 3)(x)
        assert kx.spec.kind == "add"
        got = KroneckerFusedAddedDiagLinearOperator(KroneckerFusedLinearOperator(kx, ktt), noise).to_dense_differentiable()
        os_, ls = float(inner.outputscale.detach()), inner.base_kernel.lengthscale.detach().double().reshape(-1)
        want = torch.kron(os_ * add_cov(kind, x, x, ls), ktt.double()) + torch.diag(noise.double().repeat(14))
        assert got.requires_grad and _abs_err(got.detach(), want) / float(want.abs().max()) < 4e-6


def test_additive_native_truth_table():
    import gpytorch_amd as g
    from gpytorch_amd.kernels import additive_native

    R, M, S = g.kernels.RBFKernel, g.kernels.MaternKernel, g.kernels.ScaleKernel
    x4, x9 = torch.rand(12, 4), torch.rand(12, 9)
    for d in range(2, 9):
        x = torch.rand(10, d)
        assert additive_native(_asq(R(), d), x)
        assert additive_native(_asq(R(ard_num_dims=d), d), x, torch.rand(7, d))
        for nu in (0.5, 1.5, 2.5):
            assert additive_native(_asq(M(nu=nu, ard_num_dims=d), d), x)
            assert additive_native(_asq(S(M(nu=nu)), d), x)
    yes = _asq(S(R(ard_num_dims=4)), 4)
    assert additive_native(yes, x4) and additive_native(yes, x4, None) and additive_native(yes, x4, x4)
    no = [
        ("float64 inputs", _asq(R(), 4), x4.double(), None, {}),
        ("float64 model", _asq(R(), 4).double(), x4, None, {}),
        ("float64 x2", _asq(R(), 4), x4, x4.double(), {}),
        ("input batch", _asq(R(), 4), torch.rand(2, 12, 4), None, {}),
        ("x2 batch", _asq(R(), 4), x4, torch.rand(2, 12, 4), {}),
        ("kernel batch", _asq(R(batch_shape=torch.Size([2])), 4), x4, None, {}),
        ("d = 9", _asq(R(), 9), x9, None, {}),
        ("d != num_dims", _asq(R(), 5), x4, None, {}),
        ("rq base", _asq(g.kernels.RQKernel(), 4), x4, None, {}),
        ("periodic base", _asq(g.kernels.PeriodicKernel(), 4), x4, None, {}),
        ("pp base", _asq(g.kernels.PiecewisePolynomialKernel(), 4), x4, None, {}),
        ("batched ScaleKernel", _asq(S(R(), batch_shape=torch.Size([2])), 4), x4, None, {}),
        ("two ScaleKernels", _asq(S(S(R())), 4), x4, None, {}),
        ("base with active_dims", _asq(R(active_dims=[0]), 4), x4, None, {}),
        ("last_dim_is_batch", _asq(R(), 4), x4, None, {"last_dim_is_batch": True}),
        ("inputs that require grad", _asq(R(), 4), x4.clone().requires_grad_(True), None, {}),
    ]
    for name, kern, a, b, kw in no:
        assert additive_native(kern, a, b, **kw) is False, name
    # pure: the answer does not depend on where the tensors live -- a host call of the rule never touches a device
    assert additive_native(yes, x4) is True


def test_api_errors_delegation_and_operator():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd import operators
    from gpytorch_amd.kernels import AdditiveStructureKernel, additive_dense, additive_native

    assert all(n in g.kernels.__all__ for n in ("AdditiveStructureKernel", "additive_native", "additive_dense"))
    assert additive_dense is g.kernels.additive_dense and additive_native is g.kernels.additive_native
    with pytest.warns(DeprecationWarning, match="AdditiveStructureKernel is deprecated"):
        kern = AdditiveStructureKernel(g.kernels.RBFKernel(ard_num_dims=4), num_dims=4)
    assert kern.num_dims == 4 and kern.is_stationary and kern.active_dims is None
    assert _asq(g.kernels.RBFKernel(), 3, active_dims=[0, 2, 3]).active_dims.tolist() == [0, 2, 3]
    x = torch.rand(15, 4)
    with pytest.raises(RuntimeError, match="does not accept the last_dim_is_batch argument"):
        kern(x, last_dim_is_batch=True)
    # delegation
    assert kern.prediction_strategy is kern.base_kernel.prediction_strategy
    ski = g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=8, num_dims=1)
    assert _asq(ski, 2).prediction_strategy is ski.prediction_strategy and _asq(ski, 2).is_stationary == ski.is_stationary
    assert kern.num_outputs_per_input(x, x) == 1
    assert _asq(g.kernels.RBFKernelGrad(), 2).num_outputs_per_input(torch.rand(5, 1), torch.rand(5, 1)) == 2
    # the native operator (built without a device): kind, code, expanded lengthscale, d x outputscale in the scale slot
    for kind in FAMILIES:
        for ard in (False, True):
            base = _base(g, kind, ard_num_dims=4 if ard else None)
            base.lengthscale = torch.tensor([[0.2, 0.25, 0.3, 0.35]]) if ard else 0.3
            inner = g.kernels.ScaleKernel(base)
            inner.outputscale = 1.7
            op = _asq(inner, 4)(x)
            assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "add"
            assert op.spec.code == B.KIND_IDS[kind] == B.add_code(kind) and op.spec.param is None and op.spec.param_value() == op.spec.code
            assert op.x1 is op.x2 and op.shape == (15, 15) and op.lengthscale.shape == (1, 4) and op.lengthscale.requires_grad
            assert torch.allclose(op.lengthscale.detach(), base.lengthscale.detach().expand(1, 4))
            assert abs(float(op.outputscale.detach()) - 4 * 1.7) < 1e-5 and op.outputscale.requires_grad
            assert torch.allclose(op.spec.shift, x.mean(0))
            # a single lengthscale receives the sum of the per-dimension gradients through the expansion
            (gl,) = torch.autograd.grad(op.lengthscale.sum(), base.raw_lengthscale)
            assert gl.shape == base.raw_lengthscale.shape
            bare = _asq(base, 4)(x, torch.rand(9, 4))
            assert bare.shape == (15, 9) and abs(float(bare.outputscale) - 4.0) < 1e-6 and not bare.outputscale.requires_grad
            # diag of one input: d x scale, no launch
            dg = _asq(inner, 4)(x, diag=True)
            assert dg.shape == (15,) and torch.allclose(dg, torch.full((15,), 4 * 1.7))
            assert torch.allclose(_asq(base, 4)(x, diag=True), torch.full((15,), 4.0))
            # diag of two different inputs: the dense branch
            x2 = torch.rand(15, 4)
            dd = _asq(inner, 4)(x, x2, diag=True)
            want = 1.7 * add_cov(kind, x, x2, base.lengthscale.detach().reshape(-1), diag=True)
            assert float((dd.detach().double() - want).abs().max()) < 4e-6
            # an outer ScaleKernel multiplies into the same slot
            outer = g.kernels.ScaleKernel(_asq(inner, 4))
            outer.outputscale = 0.5
            oo = outer(x)
            assert isinstance(oo, operators.FusedKernelLinearOperator) and oo.spec.kind == "add" and abs(float(oo.outputscale.detach()) - 0.5 * 4 * 1.7) < 1e-5
    # d = 1: the base kernel's own operator
    one = _asq(g.kernels.MaternKernel(nu=1.5), 1)(torch.rand(9, 1))
    assert isinstance(one, operators.FusedKernelLinearOperator) and one.spec.kind == "matern32"
    # + with other fused kernels: a sum of fused operators
    from gpytorch_amd.composite import SumFusedLinearOperator

    both = (_asq(g.kernels.RBFKernel(), 4) + g.kernels.ScaleKernel(g.kernels.RBFKernel()))(x)
    assert isinstance(both, SumFusedLinearOperator)
    # declined calls: DenseLinearOperator of additive_dense (float32 on the host: other base kernels densify through their own operators, on the device)
    x64 = x.double()
    out = _asq(g.kernels.RBFKernel().double(), 4)(x64)
    assert isinstance(out, operators.DenseLinearOperator)
    assert float((operators.to_dense(out).detach() - add_cov("rbf", x64, x64, [0.6931471805599453])).abs().max()) < 1e-12


def test_code_rule_and_python_refusals():
    from gpytorch_amd import backend as B

    assert B.KIND_IDS["add"] == 8 and B.ADD_BASE_KINDS == FAMILIES and (B.ADD_MIN_DIM, B.ADD_MAX_DIM) == (2, 8)
    for i, kind in enumerate(FAMILIES):
        assert B.add_code(kind) == i == B.add_code_check(i) == B.add_code_check(float(i), 5)
    for bad in ("rq", "pp", "prod", "add"):
        with pytest.raises(ValueError, match="additive family"):
            B.add_code(bad)
    for bad in (-1, 4, 1.5, 8):
        with pytest.raises(ValueError, match="additive family"):
            B.add_code_check(bad)
    for d in (1, 9, 0):
        with pytest.raises(ValueError, match="additive family"):
            B.add_code_check(2, d)
    xp = B.PreparedPoints(torch.zeros(8, 4), 8, 3, 4, "add", 3)
    assert B.prep_coef_of(xp) == B.prep_coef("matern52")
    assert B.kind_args(xp) == (8, 3.0)


def test_selection_policy_for_prepared_additive_clouds():
    """kv_flags / far_cull / grad_gram_ok / fused_f64 / f64_widenable on CPU-built prepared clouds (padding columns NaN, as prep_points leaves them): one
    kernel, whatever the settings and the test overrides say, and nothing that would reduce over the padded rows."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(1)
    xp = torch.full((5000, 4), float("nan"))
    xp[:, :3] = 300.0 * torch.rand(5000, 3, generator=gen)
    p = B.PreparedPoints(xp, 5000, 3, 4, "add", 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for t in (1, 4, 5, 33, 65, 140):
            assert B.kv_flags(p, p, t) == B.KV_SPLIT
        with g.settings.split_contraction(False):
            assert B.kv_flags(p, p, 11) == B.KV_SPLIT
        old = B.FORCE_KV_FLAGS
        try:
            B.FORCE_KV_FLAGS = 0
            assert B.kv_flags(p, p, 11) == B.KV_SPLIT
            B.FORCE_KV_FLAGS = B.KV_GRAM
            assert B.kv_flags(p, p, 11) == B.KV_SPLIT
        finally:
            B.FORCE_KV_FLAGS = old
        assert p._sorted is None and p._zmax2 is None              # no SortedView, no norm of the padded rows
        assert B.far_cull(p, p) is None
        with g.settings.far_pair_cutoff(1e-3):
            assert B.far_cull(p, p) is None
        assert not B.grad_gram_ok(p, p)
    assert not B.f64_widenable(p)
    p64 = B.PreparedPoints(xp.double(), 5000, 3, 4, "add", 0)
    assert not B.fused_f64(p64, p64)


def _err(h):
    return h.gpamd_last_error()


def test_abi_refusals_before_any_launch():
    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    ADD, SPLIT = 8, 8
    ok = 3.0                                                        # Matern-5/2 base
    # a bad base id, d = 1 and d = 9: every accepting entry point that knows d
    bad = [(4.0, 3), (-1.0, 3), (1.5, 3), (22.0, 3), (ok, 1), (ok, 9), (0.0, 1), (0.0, 9)]
    for code, d in bad:
        dp = (d + 3) // 4 * 4
        word = b"base family" if code not in (ok, 0.0) else b"2..8"
        assert h.gpamd_prep_points_f32(ADD, code, None, 5, d, d, None, 1, None, None, dp, None) == -1
        assert _err(h).startswith(b"prep_points:") and word in _err(h), (code, d, _err(h))
        assert h.gpamd_kv_partials_f32(ADD, code, None, 300, None, 300, d, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1
        assert _err(h).startswith(b"kv:") and word in _err(h), (code, d, _err(h))
        assert h.gpamd_kv_f32(ADD, code, None, 300, None, 300, d, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
        assert _err(h).startswith(b"kv:") and word in _err(h), (code, d, _err(h))
    for d in (1, 9, 10):
        assert h.gpamd_kv_plan(ADD, 2000, 2000, d, 11, SPLIT, 2000, None, None, None) == -1 and b"2..8" in _err(h)
    # entry points that see the padded stride only: what the code alone says
    gargs = (None, 1000, None, 1000, 4, None, 1000, None, 1000, 8, 0, None, None, 0, None, None, None, None, None, 0.0, None, 0)
    for code in (4.0, -1.0, 1.5, 22.0):
        assert h.gpamd_kernel_rows_f32(ADD, code, None, None, 3, None, 10, 4, None, None, 12, None) == -1
        assert _err(h).startswith(b"kernel_rows:") and b"base family" in _err(h)
        assert h.gpamd_kernel_dense_f32(ADD, code, None, 10, None, 10, 4, None, None, 12, None) == -1
        assert _err(h).startswith(b"kernel_dense:") and b"base family" in _err(h)
        assert h.gpamd_kernel_diag_f32(ADD, code, None, None, 10, 4, None, None, None) == -1
        assert _err(h).startswith(b"kernel_diag:") and b"base family" in _err(h)
        assert h.gpamd_pivoted_cholesky_f32(ADD, code, None, 100, 4, None, 5, 1e-3, None, 100, None, None, None, None) == -1
        assert _err(h).startswith(b"pivoted_cholesky:") and b"base family" in _err(h)
        assert h.gpamd_kv_grad_param_far_f32(ADD, code, *gargs) == -1
        assert _err(h).startswith(b"kv_grad:") and b"base family" in _err(h)
    # ... and a stride that cannot belong to d in 2..8
    assert h.gpamd_kernel_dense_f32(ADD, ok, None, 10, None, 10, 12, None, None, 12, None) == -1 and b"stride 4 or 8" in _err(h)
    assert h.gpamd_kernel_rows_f32(ADD, ok, None, None, 3, None, 10, 12, None, None, 12, None) == -1 and b"stride 4 or 8" in _err(h)
    assert h.gpamd_kernel_diag_f32(ADD, ok, None, None, 10, 12, None, None, None) == -1 and _err(h).startswith(b"kernel_diag:")
    assert h.gpamd_pivoted_cholesky_f32(ADD, ok, None, 100, 12, None, 5, 1e-3, None, 100, None, None, None, None) == -1 and b"stride 4 or 8" in _err(h)
    g12 = gargs[:4] + (12,) + gargs[5:]
    assert h.gpamd_kv_grad_param_far_f32(ADD, ok, *g12) == -1 and b"stride 4 or 8" in _err(h)
    # the derivative: per-dimension sums only (iso = 1 refused), no culling; a valid call gets as far as the workspace bound
    giso = gargs[:10] + (1,) + gargs[11:]
    assert h.gpamd_kv_grad_param_far_f32(ADD, ok, *giso) == -1 and b"iso must be 0" in _err(h)
    gcut = gargs[:19] + (1.0,) + gargs[20:]
    assert h.gpamd_kv_grad_param_far_f32(ADD, ok, *gcut) == -1 and b"not culled" in _err(h)
    assert h.gpamd_kv_grad_param_far_f32(ADD, ok, *gargs) == -3 and _err(h).startswith(b"kv_grad:")
    g8 = gargs[:4] + (8,) + gargs[5:]
    assert h.gpamd_kv_grad_param_far_f32(ADD, ok, *g8) == -3
    # the product itself: GPAMD_KV_SPLIT is required, sq_cutoff must be 0; a valid call gets as far as the shape checks (ldv % 4)
    for flags in (0, 1):
        assert h.gpamd_kv_plan(ADD, 2000, 2000, 3, 11, flags, 2000, None, None, None) == -1
        assert _err(h).startswith(b"kv_plan:") and b"GPAMD_KV_SPLIT" in _err(h)
        assert h.gpamd_kv_partials_f32(ADD, ok, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, flags, None, None) == -1
        assert _err(h).startswith(b"kv:") and b"GPAMD_KV_SPLIT" in _err(h)
        assert h.gpamd_kv_f32(ADD, ok, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, flags, None) == -1
        assert _err(h).startswith(b"kv:") and b"GPAMD_KV_SPLIT" in _err(h)
    rc = h.gpamd_kv_partials_far_f32(ADD, ok, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None, None, None, None, None,
                                     4.0, None, 0)
    assert rc == -1 and _err(h).startswith(b"kv:") and b"not culled" in _err(h)
    rc = h.gpamd_kv_partials_f32(ADD, ok, None, 300, None, 300, 3, None, None, 302, 11, None, 300, 1, 384, SPLIT, None, None)
    assert rc == -1 and b"leading dimensions" in _err(h)
    # every other entry point that takes a kind refuses the family, with the text it has for an unknown kind
    assert h.gpamd_prep_points_f64(ADD, ok, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and _err(h).startswith(b"prep_points_f64:")
    assert h.gpamd_kv_partials_f64(ADD, ok, None, 300, None, 300, 4, None, 300, 11, None, 300, 1, 384, None, None) == -1 and _err(h).startswith(b"kv_partials_f64:")
    assert h.gpamd_kernel_rows_f64(ADD, ok, None, None, 0, 3, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_diag_f64(ADD, ok, None, None, 10, 4, None, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_grad_f32(ADD, *gargs[:15]) == -1 and _err(h).startswith(b"kv_grad:")
    rc = h.gpamd_kv_grad2_f32(ADD, ok, None, 1000, None, 1000, 3, None, None, 1000, None, 1000, 8, 0, None, None, 1000, None, 0, None, 0, 0, None, 0, None)
    assert rc == -2 and _err(h).startswith(b"kv_grad2:")
    rc = h.gpamd_kv_grad2_far_f32(ADD, ok, None, 1000, None, 1000, 3, None, None, 1000, None, 1000, 8, 0, None, None, 1000, None, 0, None, 0, 0, None, 0, None,
                                  None, None, None, None, 0.0, None, 0)
    assert rc == -2 and _err(h).startswith(b"kv_grad2:")
    import ctypes as C

    kp = (C.c_float * 2)(ok, ok)
    assert h.gpamd_kernel_dense_batched_f32(ADD, kp, None, 5, None, 5, 4, 2, None, None, None, 8, None) == -1 and b"unknown kind" in _err(h)
    # kind 7 stays refused where it was, kinds beyond the new one stay unknown
    assert h.gpamd_prep_points_f32(7, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_f32(7, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
    assert h.gpamd_kv_grad_param_far_f32(7, 0.0, *gargs) == -1 and _err(h).startswith(b"kv_grad: bad arguments")
    assert h.gpamd_kernel_dense_f32(7, 0.0, None, 10, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    for kind in (9, 31, 32, 40, -1):
        assert h.gpamd_prep_points_f32(kind, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
        assert h.gpamd_kv_plan(kind, 2000, 2000, 3, 11, SPLIT, 2000, None, None, None) == -1
        assert h.gpamd_kv_partials_f32(kind, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1 and b"unknown kind" in _err(h)
        assert h.gpamd_kv_grad_param_far_f32(kind, 0.0, *gargs) == -1


def test_kv_plan_covers_fills_and_reserves_planes():
    """The plan covers the contracted index and ALWAYS holds the f16 planes of V -- one 32-row plane pair per column group of 32 (+ 1), from one
    column on, whatever flags ride along with GPAMD_KV_SPLIT -- for every d in 2..8 (d = 7 has kernels of its own: no rounding up to 8)."""
    from gpytorch_amd import backend as B

    for n, m, t in [(2000, 2000, 11), (100_000, 100_000, 65), (10_000, 100_000, 1), (257, 300, 140), (2000, 2000, 32), (2000, 2000, 33), (2000, 2000, 34)]:
        ld = B.round_up(n, 4)
        for d in range(2, 9):
            seen = set()
            for flags in (B.KV_SPLIT, B.KV_GRAM | B.KV_SPLIT, B.KV_SPLIT | B.KV_WIDE):
                S, jc, ws = B.kv_plan("add", n, m, d, t, flags, ld)
                seen.add((S, jc, ws))
                assert S >= 1 and jc % 128 == 0 and S * jc >= m and (S - 1) * jc < m
                slabs = S * t * ld
                ldh = (m + 127) // 128 * 128
                groups, g0 = 0, 0
                while g0 < t:
                    g0 += (t - g0) if t - g0 <= 33 else 32
                    groups += 1
                rows = 32 * groups
                assert ws >= slabs + rows * ldh and ws <= slabs + rows * ldh + 2 * (2 * t + 64) + 8 and ws % 4 == 0, (n, m, t, d, ws, slabs, rows)
            assert len(seen) == 1
