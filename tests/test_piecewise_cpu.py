"""CPU: the piecewise-polynomial family (``kernels.PiecewisePolynomialKernel``, ``KIND_PP``) -- the float64 restatement the GPU tests use as
oracle against outputs of the reference's own code, the kernel class, the culling policy on CPU-built prepared clouds and the C ABI's checks."""
import os

import numpy as np
import pytest
import torch

from tests.piecewise_ref import pp_cov, pp_j

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "piecewise_values.npz")
CASES = "abcdefgh"


def test_restatement_matches_reference_outputs():
    """tests/golden/piecewise_values.npz (make_piecewise_golden.py: the reference's forward, _fmax and _get_cov executed on small clouds).  float64
    fixtures: 1e-12.  float32 fixtures: the rule of test_gpu_kv.py::test_golden_kernel_values -- the reference forms distances through the Gram trick
    in the fixture's dtype, 5e-5, and 3e-4 where k has a cusp in r at zero (there Matern nu = 1/2, here q = 0)."""
    z = np.load(GOLDEN)
    seen = set()
    for name in CASES:
        x1, x2, ls = (torch.from_numpy(z[f"{name}_{k}"]) for k in ("x1", "x2", "ls"))
        f32 = z[f"{name}_x1"].dtype == np.float32
        seen.add((x1.shape[1], f32, ls.numel() > 1))
        r = (x1.double().unsqueeze(1) / ls.double() - x2.double().unsqueeze(0) / ls.double()).norm(dim=-1)
        assert 0.1 < float((r < 1).double().mean()) < 0.9          # pairs on both sides of the support radius
        for q in range(4):
            ref = torch.from_numpy(z[f"{name}_K{q}"]).double()
            err = float((pp_cov(x1, x2, ls, q) - ref).abs().max())
            tol = (3e-4 if q == 0 else 5e-5) if f32 else 1e-12
            print(name, q, err)
            assert err < tol, (name, q, err)
            assert bool((ref[r > 1 + 1e-3] == 0).all())
    assert {d for d, _, _ in seen} == {1, 2, 3, 5, 10} and {f for _, f, _ in seen} == {True, False} and {a for _, _, a in seen} == {True, False}


def test_kernel_class_shape_and_state():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    PP = g.kernels.PiecewisePolynomialKernel
    for bad in (-1, 4, 1.5, None):
        with pytest.raises(ValueError, match="q expected to be 0, 1, 2 or 3"):
            PP(q=bad)
    assert PP().q == 2
    for q in range(4):
        k = PP(q=q)
        for d in (1, 2, 3, 5, 10, 16, 32):
            code = k.shape_code(d)
            assert code == 4 * pp_j(d, q) + q == B.pp_code(d, q) and float(np.float32(code)) == code
            assert B.pp_code_check(code) == code
        spec = k._make_spec(torch.zeros(7, 5))
        assert spec.kind == "pp" and spec.code == 4 * pp_j(5, q) + q and spec.param is None and spec.param_value() == spec.code
        assert spec.with_dvec(torch.zeros(7)).code == spec.code
    # active_dims: D is what the kernel sees
    k = PP(q=1, active_dims=(0, 2))
    assert k._make_spec(k._select(torch.zeros(6, 5))).code == 4 * pp_j(2, 1) + 1
    # last_dim_is_batch: one-dimensional members, j from the original last dimension (the reference's D = x1.shape[1])
    seen = []
    k = PP(q=2)
    orig = k._make_spec
    k._make_spec = lambda x1, *a, **kw: seen.append((x1.shape[-1], orig(x1, *a, **kw).code)) or orig(x1, *a, **kw)
    k(torch.rand(9, 4), last_dim_is_batch=True)
    assert seen and all(w == 1 and c == 4 * pp_j(4, 2) + 2 for w, c in seen)
    # no parameter beyond the lengthscale
    assert sorted(PP(q=3).state_dict()) == sorted(g.kernels.RBFKernel().state_dict())
    assert sorted(PP(ard_num_dims=3).state_dict()) == sorted(g.kernels.RBFKernel(ard_num_dims=3).state_dict())
    assert "PiecewisePolynomialKernel" in g.kernels.__all__
    for bad in (3, 4 * 1 + 1, 4 * 3 + 3, -4, 8.5):
        with pytest.raises(ValueError):
            B.pp_code_check(bad)
    assert B.KIND_IDS["pp"] == 5 and B.prep_coef("pp") == 1.0


def test_dense_torch_branch_matches_restatement():
    from gpytorch_amd.kernels import pp_dense

    g = torch.Generator().manual_seed(3)
    x = torch.rand(40, 3, generator=g, dtype=torch.float64)
    ls = torch.tensor([0.6])
    r = (x.unsqueeze(1) / ls - x.unsqueeze(0) / ls).norm(dim=-1)
    for q in range(4):
        assert float((pp_dense(r, 4 * pp_j(3, q) + q) - pp_cov(x, x, ls, q)).abs().max()) < 1e-14


def _cloud(n, scale, kind, param):
    from gpytorch_amd import backend as B

    g = torch.Generator().manual_seed(5)
    base = torch.rand(n, 3, generator=g)
    xp = torch.zeros(n, 4)
    xp[:, :3] = (base - base.mean(0)) * scale
    return B.PreparedPoints(xp, n, 3, 4, kind, param)


def test_far_cull_policy_for_compact_support():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    S = g.settings
    code = B.pp_code(3, 2)
    p = _cloud(4096, 20.0, "pp", code)
    assert S.far_pair_cutoff.value() is None and S.compact_support_culling.on()
    assert B.far_sq_cutoff("pp", 1e-7, code) == 1.0 and B.far_sq_cutoff("pp", 0.5, code) == 1.0
    assert B.far_cull(p, p) == 1.0                                  # exact: no tolerance, no user setting
    with S.far_pair_cutoff(1e-3):
        assert B.far_cull(p, p) == 1.0                              # the user's eps plays no part
    with S.compact_support_culling(False):
        assert B.far_cull(p, p) is None
        with S.far_pair_cutoff(1e-3):
            assert B.far_cull(p, p) is None
    assert B.far_cull(p, p) == 1.0
    small = _cloud(B.FAR_MIN_POINTS - 1, 20.0, "pp", code)
    assert B.far_cull(small, small) is None
    narrow = _cloud(4096, 0.5, "pp", code)                          # the whole cloud inside one support radius: nothing to drop
    assert B.far_cull(narrow, narrow) is None
    # the infinite-support families are untouched: off by default, the eps rule under the setting, whatever the new flag says
    r = _cloud(4096, 20.0, "rbf", None)
    assert B.far_cull(r, r) is None
    with S.compact_support_culling(False):
        assert B.far_cull(r, r) is None
    with S.far_pair_cutoff(1e-7):
        assert B.far_cull(r, r) == B.far_sq_cutoff("rbf", 1e-7)
        with S.compact_support_culling(False):
            assert B.far_cull(r, r) == B.far_sq_cutoff("rbf", 1e-7)
    assert B.cusp_at_origin(_cloud(8, 1.0, "pp", B.pp_code(3, 0))) and not B.cusp_at_origin(p) and B.cusp_at_origin(_cloud(8, 1.0, "matern12", None))


def test_abi_accepts_the_new_kind_and_checks_its_code():
    import ctypes as C

    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5
    S, jc, ws = C.c_int(0), C.c_int(0), C.c_int64(0)
    assert h.gpamd_kv_plan(5, 2000, 2000, 3, 11, 0, 2000, C.byref(S), C.byref(jc), C.byref(ws)) == 0 and S.value >= 1
    assert h.gpamd_kv_plan(5, 2000, 2000, 3, 11, 1 | 8, 2000, C.byref(S), C.byref(jc), C.byref(ws)) == 0 and jc.value % 128 == 0
    assert h.gpamd_kv_plan(6, 2000, 2000, 3, 11, 0, 2000, C.byref(S), C.byref(jc), C.byref(ws)) == -1
    for bad in (3.0, 4.0 * 1 + 1, 4.0 * 3 + 3, 18.5, -2.0):           # q = 3 with j = 0; j = 1 < q + 1; j = 3 < 4; no integer; negative
        assert h.gpamd_prep_points_f64(5, bad, None, 5, 2, 2, None, 1, None, None, 4, None) == -1
        assert b"piecewise-polynomial shape code" in h.gpamd_last_error()
        assert h.gpamd_prep_points_f32(5, bad, None, 5, 2, 2, None, 1, None, None, 4, None) == -1
        assert b"piecewise-polynomial shape code" in h.gpamd_last_error()
    assert h.gpamd_prep_points_f64(6, 14.0, None, 5, 2, 2, None, 1, None, None, 4, None) == -1 and b"bad shape" in h.gpamd_last_error()
    assert h.gpamd_kernel_dense_batched_f32(5, None, None, 5, None, 5, 4, 2, None, None, None, 8, None) == -1 and b"kparam" in h.gpamd_last_error()
    # the direct-difference derivative with the shape code (additive entry point): the code is checked, RQ has no kernel there, the workspace bound
    args = (None, 1000, None, 1000, 4, None, 1000, None, 1000, 8, 0, None, None, 0, None, None, None, None, None, 0.0, None, 0)
    assert h.gpamd_kv_grad_param_far_f32(5, 5.0, *args) == -1 and b"piecewise-polynomial shape code" in h.gpamd_last_error()
    assert h.gpamd_kv_grad_param_far_f32(4, 1.5, *args) == -1 and h.gpamd_last_error().startswith(b"kv_grad:")
    assert h.gpamd_kv_grad_param_far_f32(5, 14.0, *args) == -3 and h.gpamd_last_error().startswith(b"kv_grad:")
    assert h.gpamd_kv_grad_f32(5, *args[:15]) == -1                      # the entry point without kparam keeps to the families without one
    # q = 0 has a cusp at r = 0: the Gram-form derivative kernel refuses it before any launch
    rc = h.gpamd_kv_grad2_f32(5, 8.0, None, 1000, None, 1000, 3, None, None, 1000, None, 1000, 8, 1, None, None, 1000, None, 0, None, 0, 0, None, 0, None)
    assert rc == -2 and b"q = 0" in h.gpamd_last_error()
