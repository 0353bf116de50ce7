"""CPU: the product family (``KIND_PROD`` / ``GPAMD_PROD`` = 6, ``kernels.product_factors``) -- its code, every refusal of the C ABI before any launch,
the launch plan, and which products ``ProductKernel`` recognises.  Oracle of the values: tests/product_ref.py."""
import ctypes as C
import itertools

import pytest
import torch

from tests.product_ref import FAMILIES, PAIRS, factor_cov, prod_cov


def _admitted():
    """Every (K_A, K_B, D_A, D_B) the code rule admits: 72."""
    return [(ka, kb, da, db) for ka, kb in PAIRS for da in (1, 2, 3) for db in (1, 2, 3) if ka != kb or da <= db]


def test_code_round_trip_and_python_refusals():
    from gpytorch_amd import backend as B

    assert B.KIND_IDS["prod"] == 6 and B.PROD_FACTOR_KINDS == FAMILIES
    adm = _admitted()
    assert len(adm) == 72 and len(PAIRS) == 9
    for ka, kb, da, db in adm:
        code = B.prod_code(ka, kb, da)
        assert code == ka + 4 * kb + 16 * da and float(torch.tensor(code, dtype=torch.float32)) == code
        assert B.prod_decode(code) == (ka, kb, da) and B.prod_code_check(code, da + db) == code
        coefs = B.prod_prep_coefs(code, da + db)
        assert coefs == [B.prep_coef(FAMILIES[ka])] * da + [B.prep_coef(FAMILIES[kb])] * db
    bad_codes = [0 + 4 * 0 + 16 * 1,      # RBF x RBF
                 2 + 4 * 1 + 16 * 1,      # K_A > K_B
                 1 + 4 * 2 + 16 * 0,      # D_A = 0
                 1 + 4 * 2 + 16 * 4,      # D_A = 4
                 21.5, -3, 64]
    for bad in bad_codes:
        with pytest.raises(ValueError, match="product code"):
            B.prod_code_check(bad)
    for code, d in [(B.prod_code(1, 2, 2), 2), (B.prod_code(1, 2, 2), 6), (B.prod_code(2, 2, 2), 3), (B.prod_code(0, 3, 3), 7)]:
        with pytest.raises(ValueError, match="product code"):      # D_B = 0; D_B = 4; equal families with D_A > D_B; D_B = 4
            B.prod_code_check(code, d)
    with pytest.raises(ValueError):
        B.prod_code(2, 1, 1)
    # the per-dimension preparation factor: prep_coef_of must not be used for this family
    xp = B.PreparedPoints(torch.zeros(8, 4), 8, 3, 4, "prod", B.prod_code(0, 3, 1))
    with pytest.raises(ValueError, match="prod_prep_coefs"):
        B.prep_coef_of(xp)


def test_selection_policy_for_prepared_products():
    """kv_flags / far_cull / grad_gram_ok / fused_f64 on CPU-built prepared clouds: one kernel, whatever the settings and the test overrides say."""
    import warnings

    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(1)
    xp = torch.zeros(5000, 4)
    xp[:, :3] = 300.0 * torch.rand(5000, 3, generator=gen)      # far outside the Gram policy: a single family would warn and sort
    p = B.PreparedPoints(xp, 5000, 3, 4, "prod", B.prod_code(0, 3, 1))
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
        assert p._sorted is None                                    # no SortedView was built
        assert B.far_cull(p, p) is None
        with g.settings.far_pair_cutoff(1e-3):
            assert B.far_cull(p, p) is None
        assert not B.grad_gram_ok(p, p)
    p64 = B.PreparedPoints(xp.double(), 5000, 3, 4, "prod", B.prod_code(0, 3, 1))
    assert not B.fused_f64(p64, p64)
    r64 = B.PreparedPoints(xp.double(), 5000, 3, 4, "rbf", None)
    assert B.fused_f64(r64, r64)


def _err(h):
    return h.gpamd_last_error()


def test_abi_refusals_before_any_launch():
    from gpytorch_amd import backend as B
    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    PROD = 6
    ok = float(B.prod_code(0, 3, 1))                                # RBF(1) x Matern-5/2(2): d = 3
    # (code, d) pairs every accepting entry point that knows d must refuse
    bad = [(16.0 * 1 + 0, 2), (2.0 + 4 * 1 + 16, 2), (1.0 + 4 * 2, 2), (1.0 + 4 * 2 + 64, 6), (21.5, 3), (-3.0, 3), (64.0, 3),
           (float(B.prod_code(1, 2, 2)), 2), (float(B.prod_code(1, 2, 2)), 6), (float(B.prod_code(2, 2, 2)), 3), (float(B.prod_code(0, 3, 3)), 7)]
    for code, d in bad:
        dp = 4 if d <= 4 else 8
        assert h.gpamd_prep_points_f32(PROD, code, None, 5, d, d, None, 1, None, None, dp, None) == -1
        assert _err(h).startswith(b"prep_points:") and b"product code" in _err(h), (code, d, _err(h))
        assert h.gpamd_kv_partials_f32(PROD, code, None, 300, None, 300, d, None, None, 300, 11, None, 300, 1, 384, 8, None, None) == -1
        assert _err(h).startswith(b"kv:") and b"product code" in _err(h), (code, d, _err(h))
        assert h.gpamd_kv_f32(PROD, code, None, 300, None, 300, d, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, 8, None) == -1
        assert _err(h).startswith(b"kv:") and b"product code" in _err(h), (code, d, _err(h))
    # entry points that see the padded stride only: what the code alone says
    gargs = (None, 1000, None, 1000, 4, None, 1000, None, 1000, 8, 0, None, None, 0, None, None, None, None, None, 0.0, None, 0)
    for code in (16.0, 2.0 + 4 * 1 + 16, 1.0 + 4 * 2, 1.0 + 4 * 2 + 64, 21.5, -3.0, 64.0):
        assert h.gpamd_kernel_rows_f32(PROD, code, None, None, 3, None, 10, 4, None, None, 12, None) == -1
        assert _err(h).startswith(b"kernel_rows:") and b"product code" in _err(h)
        assert h.gpamd_kernel_dense_f32(PROD, code, None, 10, None, 10, 4, None, None, 12, None) == -1
        assert _err(h).startswith(b"kernel_dense:") and b"product code" in _err(h)
        assert h.gpamd_kernel_diag_f32(PROD, code, None, None, 10, 4, None, None, None) == -1
        assert _err(h).startswith(b"kernel_diag:") and b"product code" in _err(h)
        assert h.gpamd_pivoted_cholesky_f32(PROD, code, None, 100, 4, None, 5, 1e-3, None, 100, None, None, None, None) == -1
        assert _err(h).startswith(b"pivoted_cholesky:") and b"product code" in _err(h)
        assert h.gpamd_kv_grad_param_far_f32(PROD, code, *gargs) == -1
        assert _err(h).startswith(b"kv_grad:") and b"product code" in _err(h)
    # ... and a stride that cannot belong to d <= 6, or that ends before the second factor begins
    assert h.gpamd_kernel_dense_f32(PROD, ok, None, 10, None, 10, 12, None, None, 12, None) == -1 and b"stride 4 or 8" in _err(h)
    assert h.gpamd_kernel_diag_f32(PROD, ok, None, None, 10, 12, None, None, None) == -1 and _err(h).startswith(b"kernel_diag:")
    g12 = gargs[:4] + (12,) + gargs[5:]
    assert h.gpamd_kv_grad_param_far_f32(PROD, ok, *g12) == -1 and b"stride 4 or 8" in _err(h)
    # the derivative: per-dimension sums only, no culling; a valid call gets as far as the workspace bound
    giso = gargs[:10] + (1,) + gargs[11:]
    assert h.gpamd_kv_grad_param_far_f32(PROD, ok, *giso) == -1 and b"iso must be 0" in _err(h)
    gcut = gargs[:19] + (1.0,) + gargs[20:]
    assert h.gpamd_kv_grad_param_far_f32(PROD, ok, *gcut) == -1 and b"not culled" in _err(h)
    assert h.gpamd_kv_grad_param_far_f32(PROD, ok, *gargs) == -3 and _err(h).startswith(b"kv_grad:")
    # the product itself: no culling; a valid call gets as far as the shape checks (ldv % 4)
    rc = h.gpamd_kv_partials_far_f32(PROD, ok, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, 8, None, None, None, None, None, None,
                                     4.0, None, 0)
    assert rc == -1 and _err(h).startswith(b"kv:") and b"not culled" in _err(h)
    rc = h.gpamd_kv_partials_f32(PROD, ok, None, 300, None, 300, 3, None, None, 302, 11, None, 300, 1, 384, 8, None, None)
    assert rc == -1 and b"leading dimensions" in _err(h)
    # every other entry point that takes a kind refuses the family
    assert h.gpamd_prep_points_f64(PROD, ok, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and _err(h).startswith(b"prep_points_f64:")
    assert h.gpamd_kv_partials_f64(PROD, ok, None, 300, None, 300, 4, None, 300, 11, None, 300, 1, 384, None, None) == -1 and _err(h).startswith(b"kv_partials_f64:")
    assert h.gpamd_kernel_rows_f64(PROD, ok, None, None, 0, 3, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_diag_f64(PROD, ok, None, None, 10, 4, None, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_grad_f32(PROD, *gargs[:15]) == -1 and _err(h).startswith(b"kv_grad:")
    rc = h.gpamd_kv_grad2_f32(PROD, ok, None, 1000, None, 1000, 3, None, None, 1000, None, 1000, 8, 0, None, None, 1000, None, 0, None, 0, 0, None, 0, None)
    assert rc == -1 and _err(h).startswith(b"kv_grad2:") and b"product family" in _err(h)
    rc = h.gpamd_kv_grad2_far_f32(PROD, ok, None, 1000, None, 1000, 3, None, None, 1000, None, 1000, 8, 0, None, None, 1000, None, 0, None, 0, 0, None, 0, None,
                                  None, None, None, None, 0.0, None, 0)
    assert rc == -1 and _err(h).startswith(b"kv_grad2:")
    kp = (C.c_float * 2)(ok, ok)
    assert h.gpamd_kernel_dense_batched_f32(PROD, kp, None, 5, None, 5, 4, 2, None, None, None, 8, None) == -1 and b"unknown kind" in _err(h)
    # kinds beyond the new one stay unknown
    assert h.gpamd_prep_points_f32(7, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_plan(7, 2000, 2000, 3, 11, 0, 2000, None, None, None) == -1


def test_kv_plan_covers_fills_and_reserves_planes():
    """The shapes of tests/test_lib_abi.py::test_kv_plan_covers_and_fills: the plan covers the contracted index, and ALWAYS holds the f16 planes of V
    -- one 32-row plane pair per column group of 32 (+ 1), from one column on, whatever flags are passed."""
    from gpytorch_amd import backend as B

    for n, m, t in [(2000, 2000, 11), (100_000, 100_000, 65), (500_000, 500_000, 65), (1_000_000, 1_000_000, 33), (10_000, 100_000, 1), (257, 300, 140),
                    (2000, 2000, 1), (2000, 2000, 4), (2000, 2000, 32), (2000, 2000, 34), (2000, 2000, 64)]:
        ld = B.round_up(n, 4)
        seen = set()
        for d in (2, 3, 4, 5, 6):
            for flags in (B.KV_SPLIT, B.KV_GRAM | B.KV_SPLIT, B.KV_SPLIT | B.KV_WIDE):
                S, jc, ws = B.kv_plan("prod", n, m, d, t, flags, ld)
                seen.add((d, S, jc, ws))
                assert S >= 1 and jc % 128 == 0 and S * jc >= m and (S - 1) * jc < m
                slabs = S * t * ld
                ldh = (m + 127) // 128 * 128
                groups = 0
                g0 = 0
                while g0 < t:                                       # groups of 32 columns; a remainder of 33 is 32 + the extra VALU column
                    g0 += (t - g0) if t - g0 <= 33 else 32
                    groups += 1
                rows = 32 * groups
                assert ws >= slabs + rows * ldh and ws <= slabs + rows * ldh + 2 * (2 * t + 64) + 8 and ws % 4 == 0, (n, m, t, d, ws, slabs, rows)
        assert len({s[1:] for s in seen if s[0] == 3}) == 1        # flags beyond KV_SPLIT play no part
    from gpytorch_amd._lib import lib

    h = lib()
    for d in (1, 7, 10):
        assert h.gpamd_kv_plan(6, 2000, 2000, d, 11, 8, 2000, None, None, None) == -1 and b"2..6" in h.gpamd_last_error()
    # the family's one kernel is the split-contraction one: the caller asks for it (a plan without the flag would hold no planes)
    ok = float(B.prod_code(0, 3, 1))
    for flags in (0, B.KV_GRAM):
        assert h.gpamd_kv_plan(6, 2000, 2000, 3, 11, flags, 2000, None, None, None) == -1
        assert h.gpamd_last_error().startswith(b"kv_plan:") and b"GPAMD_KV_SPLIT" in h.gpamd_last_error()
        assert h.gpamd_kv_partials_f32(6, ok, None, 300, None, 300, 3, None, None, 300, 11, None, 300, 1, 384, flags, None, None) == -1
        assert h.gpamd_last_error().startswith(b"kv:") and b"GPAMD_KV_SPLIT" in h.gpamd_last_error()
        assert h.gpamd_kv_f32(6, ok, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, flags, None) == -1
        assert h.gpamd_last_error().startswith(b"kv:") and b"GPAMD_KV_SPLIT" in h.gpamd_last_error()


# ---------------------------------------------------------------------------------------------- ProductKernel recognition
def _kern(g, fam, **kw):
    return g.kernels.RBFKernel(**kw) if fam == 0 else g.kernels.MaternKernel(nu={1: 0.5, 2: 1.5, 3: 2.5}[fam], **kw)


def test_product_factors_accepts_and_orders():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd.kernels import product_factors

    x = torch.rand(20, 3)
    for fa, fb in itertools.product(range(4), range(4)):
        a, b = _kern(g, fa, active_dims=[0]), _kern(g, fb, active_dims=[1, 2])
        pf = product_factors(a * b, x)
        pr = product_factors(b * a, x)
        if fa == 0 and fb == 0:
            assert pf is None and pr is None                      # RBF x RBF: the feature path
            continue
        for got in (pf, pr):                                      # the user's order never matters
            assert got is not None
            lo, hi = (a, b) if (fa, 1) <= (fb, 2) else (b, a)
            assert got.a is lo and got.b is hi
            assert (got.ka, got.kb) == (min(fa, fb), max(fa, fb))
            assert got.code == B.prod_code(got.ka, got.kb, got.da) and got.da + got.db == 3
            assert B.prod_code_check(got.code, 3) == got.code
            assert got.scale is None
    # equal families: the one with fewer columns is A
    a, b = g.kernels.MaternKernel(nu=1.5, active_dims=[1, 2]), g.kernels.MaternKernel(nu=1.5, active_dims=[0])
    pf = product_factors(a * b, x)
    assert pf.a is b and (pf.da, pf.db) == (1, 2)
    # overlapping / coinciding column groups are gathered, not partitioned
    a, b = g.kernels.RBFKernel(), g.kernels.MaternKernel()
    pf = product_factors(a * b, x)
    assert (pf.da, pf.db) == (3, 3) and pf.a is a and pf.code == B.prod_code(0, 3, 3)
    assert torch.equal(pf.gather(x), torch.cat([x, x], -1))
    a, b = g.kernels.MaternKernel(nu=0.5, active_dims=[2, 0]), g.kernels.RBFKernel(active_dims=[0, 1], ard_num_dims=2)
    b.lengthscale = torch.tensor([[0.3, 0.7]])
    a.lengthscale = 0.5
    pf = product_factors(a * b, x)
    assert pf.a is b and torch.equal(pf.gather(x), x[:, [0, 1, 2, 0]])
    assert torch.allclose(pf.lengthscale(), torch.tensor([[0.3, 0.7, 0.5, 0.5]])) and pf.lengthscale().requires_grad
    # 1-D inputs are one column
    pf = product_factors(g.kernels.RBFKernel() * g.kernels.MaternKernel(nu=1.5), torch.rand(9))
    assert (pf.da, pf.db) == (1, 1) and pf.gather(torch.rand(9)).shape == (9, 2)
    # ScaleKernels are peeled (any nesting), nested ProductKernels flattened: the outputscales multiply into one
    s1 = g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5, active_dims=[0]))
    s2 = g.kernels.ScaleKernel(g.kernels.ProductKernel(g.kernels.ScaleKernel(g.kernels.RBFKernel(active_dims=[1, 2]))))
    s1.outputscale, s2.outputscale, s2.base_kernel.kernels[0].outputscale = 1.5, 0.5, 3.0
    pf = product_factors(g.kernels.ProductKernel(s1, s2), x)
    assert pf is not None and pf.a is s2.base_kernel.kernels[0].base_kernel and pf.b is s1.base_kernel
    assert abs(float(pf.scale.detach()) - 2.25) < 1e-6 and pf.scale.requires_grad
    pf = product_factors(g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5, active_dims=[0]) * g.kernels.RBFKernel(active_dims=[1, 2])), x)
    assert pf is not None and pf.scale is not None


def _declined(g):
    M, R = g.kernels.MaternKernel, g.kernels.RBFKernel
    x3, x5 = torch.rand(12, 3), torch.rand(12, 5)
    return [
        ("periodic member", M() * g.kernels.PeriodicKernel(), x3, {}),
        ("rq member", R(active_dims=[0]) * g.kernels.RQKernel(active_dims=[1]), x3, {}),
        ("three non-SE factors", M(nu=0.5, active_dims=[0]) * M(nu=1.5, active_dims=[1]) * M(nu=2.5, active_dims=[2]), x3, {}),
        ("two RBF and a Matern", R(active_dims=[0]) * R(active_dims=[1]) * M(active_dims=[2]), x3, {}),
        ("float64", R(active_dims=[0]) * M(active_dims=[1]), x3.double(), {}),
        ("more than three columns", R() * M(active_dims=[0]), x5, {}),
        ("input batch", R(active_dims=[0]) * M(active_dims=[1]), torch.rand(2, 12, 3), {}),
        ("kernel batch", R(active_dims=[0], batch_shape=torch.Size([2])) * M(active_dims=[1], batch_shape=torch.Size([2])), x3, {}),
        ("last_dim_is_batch", R() * M(), x3, {"last_dim_is_batch": True}),
        ("single member", g.kernels.ProductKernel(M()), x3, {}),
    ]


def _cpu_dense(op):
    """``FusedKernelLinearOperator.to_dense`` restated on the CPU (tests/product_ref.py), so that the dense branch can run without a device."""
    kind = op.spec.kind
    x1, x2, ls = op.x1.detach(), op.x2.detach(), op.lengthscale.detach().reshape(-1)
    if kind == "rq":
        alpha = float(op.spec.param.detach().reshape(-1)[0])
        z1, z2 = x1.double() / ls.double(), x2.double() / ls.double()
        k = (1 + (z1.unsqueeze(-2) - z2.unsqueeze(-3)).pow(2).sum(-1) / (2 * alpha)).pow(-alpha)
    else:
        assert kind in FAMILIES, kind
        k = factor_cov(kind, x1, x2, ls)
    k = k if op.outputscale is None else k * float(op.outputscale.detach().reshape(-1)[0])
    return k.to(x1.dtype)


def test_declined_products_keep_the_dense_path(monkeypatch):
    """Everything outside the rule returns what it returned before: a DenseLinearOperator holding the product of the members' dense matrices, and the
    product of the members' diagonals.  (The members' own ``to_dense`` is restated on the CPU for the purpose.)"""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.kernels import product_factors

    monkeypatch.setattr(operators.FusedKernelLinearOperator, "to_dense", _cpu_dense)
    for name, kern, x, params in _declined(g):
        if name == "last_dim_is_batch":
            assert product_factors(kern, x, None, True) is None, name
            continue                                               # (members under last_dim_is_batch build batches: nothing to run here)
        assert product_factors(kern, x) is None, name
        if x.dim() > 2 or any(len(k.batch_shape) for k in kern.kernels):
            continue                                               # (batches evaluate member by member on the device)
        out = kern(x)
        assert isinstance(out, operators.DenseLinearOperator), name
        want = None
        for k in kern.kernels:
            term = operators.to_dense(k(x, x))
            want = term if want is None else want * term
        assert torch.equal(operators.to_dense(out), want), name
        d = kern(x, diag=True)
        assert torch.is_tensor(d) and torch.allclose(d, torch.ones(x.shape[0], dtype=x.dtype)), name
    # the squared-exponential family keeps its feature path: one fused RBF operator
    x = torch.rand(12, 3)
    se = g.kernels.RBFKernel(active_dims=[0]) * g.kernels.PeriodicKernel(active_dims=[1]) * g.kernels.RBFKernel(active_dims=[2])
    assert product_factors(se, x) is None
    op = se(x)
    assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "rbf" and op.x1.shape[-1] == 4
    assert product_factors(g.kernels.RBFKernel() * g.kernels.RBFKernel(), x) is None


def test_recognised_product_builds_one_fused_operator():
    """The operator ``ProductKernel.forward`` builds (no device needed to build it): kind, code, gathered cloud, lengthscales, combined outputscale,
    the diagonal rules -- and its values through the CPU restatement of the factors."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd import operators

    x, x2 = torch.rand(15, 3), torch.rand(9, 3)
    for order in (0, 1):
        ka, kb = g.kernels.MaternKernel(nu=2.5, active_dims=[0]), g.kernels.RBFKernel(active_dims=[1, 2], ard_num_dims=2)
        ka.lengthscale, kb.lengthscale = 0.4, torch.tensor([[0.3, 0.6]])
        kern = g.kernels.ScaleKernel(ka * kb if order == 0 else kb * ka)
        kern.outputscale = 1.7
        op = kern(x)
        assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "prod"
        assert op.spec.code == B.prod_code(0, 3, 2) and op.spec.param is None and op.spec.param_value() == op.spec.code
        assert torch.equal(op.x1, x[:, [1, 2, 0]]) and op.x2 is op.x1 and op.shape == (15, 15)
        assert torch.allclose(op.lengthscale, torch.tensor([[0.3, 0.6, 0.4]])) and abs(float(op.outputscale) - 1.7) < 1e-6
        assert torch.allclose(op.spec.shift, x[:, [1, 2, 0]].mean(0))
        assert op.requires_grad
        r = kern(x, x2)
        assert r.shape == (15, 9) and torch.equal(r.x2, x2[:, [1, 2, 0]]) and r.spec.code == op.spec.code
        # diag: same inputs -> ones x outputscale; two different equally long inputs -> the product of the members' diagonals (needs the device)
        d = kern(x, diag=True)
        assert d.shape == (15,) and torch.allclose(d, torch.full((15,), 1.7))
        # values: gathered cloud + code against the members, restated
        K = prod_cov(0, 3, 2, op.x1, op.x1, op.lengthscale.detach().reshape(-1))
        want = factor_cov("matern52", x[:, [0]], x[:, [0]], [0.4]) * factor_cov("rbf", x[:, 1:], x[:, 1:], [0.3, 0.6])
        assert float((K - want).abs().max()) < 1e-6                # (float32 lengthscales)
    # the torch restatement used by the small dense branches
    from gpytorch_amd.kernels import stationary_dense

    z = x.double() / 0.4
    d2 = (z.unsqueeze(1) - z.unsqueeze(0)).pow(2).sum(-1)
    for fam in FAMILIES:
        assert float((stationary_dense(fam, d2) - factor_cov(fam, x, x, [0.4])).abs().max()) < 1e-9
