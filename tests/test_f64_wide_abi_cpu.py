"""CPU: the float64 product's plan and refusals for prepared strides beyond 16 (csrc/kv_f64_wide.hpp) -- no launch, no GPU."""
import ctypes as C

import pytest
import torch


@pytest.mark.parametrize("dp", [20, 512])
@pytest.mark.parametrize("n,m,t", [(130, 200, 1), (257, 600, 69), (100_000, 100_000, 11)])
def test_plan_covers_the_contracted_rows(dp, n, m, t):
    from gpytorch_amd._lib import lib

    ldo = (n + 3) // 4 * 4
    S, jc, ws = C.c_int(), C.c_int(), C.c_int64()
    assert lib().gpamd_kv_plan_f64(n, m, dp, t, ldo, C.byref(S), C.byref(jc), C.byref(ws)) == 0
    assert jc.value % 64 == 0 and S.value * jc.value >= m > (S.value - 1) * jc.value
    assert ws.value == S.value * t * ldo


@pytest.mark.parametrize("dp", [18, 516])
def test_plan_refuses_other_strides(dp):
    from gpytorch_amd._lib import lib

    S, jc, ws = C.c_int(), C.c_int(), C.c_int64()
    assert lib().gpamd_kv_plan_f64(130, 200, dp, 1, 132, C.byref(S), C.byref(jc), C.byref(ws)) == -2
    assert b"20 .. 512" in lib().gpamd_last_error()


def test_partials_refusals_before_any_launch():
    from gpytorch_amd import backend as B
    from gpytorch_amd._lib import lib

    h = lib()
    for kind, kparam in (("matern12", 0.0), ("pp", float(B.pp_code(20, 1)))):   # a cusp at the origin: not in Gram form
        assert h.gpamd_kv_partials_f64(B.KIND_IDS[kind], kparam, None, 130, None, 200, 20, None, 200, 1, None, 132, 1, 256, None, None) == -2
        assert b"Matern 3/2, 5/2" in h.gpamd_last_error()
    assert h.gpamd_kv_partials_f64(B.KIND_IDS["rbf"], 0.0, None, 130, None, 200, 20, None, 200, 1, None, 128, 1, 256, None, None) == -1   # ldo < n
    assert h.gpamd_kv_partials_f64(B.KIND_IDS["rbf"], 0.0, None, 130, None, 200, 20, None, 200, 1, None, 132, 1, 200, None, None) == -1   # jchunk % 64


def test_fused_f64_wants_device_clouds():
    from gpytorch_amd import backend as B

    xp = torch.zeros(50, 20, dtype=torch.float64)
    p = B.PreparedPoints(xp, 50, 17, 20, "rbf", None)
    assert B.FUSED_F64_WIDE_MAX_DP == 512 and B.FUSED_F64_MAX_DP == 16 and "matern12" not in B.FUSED_F64_WIDE_KINDS
    assert not B.fused_f64(p, p)
