"""The entry points of the wide direct-difference product (gpamd_kv_wide_direct_*): the plan, and every refusal before any launch -- no GPU needed."""
import ctypes as C

import pytest


def _plan(h, kind, n, m, d, t, ldo):
    S, jc, ws = C.c_int(0), C.c_int(0), C.c_int64(0)
    return h.gpamd_kv_wide_direct_plan(kind, n, m, d, t, ldo, C.byref(S), C.byref(jc), C.byref(ws)), S.value, jc.value, ws.value


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("n,m,t", [(77, 131, 1), (3000, 3000, 12), (640, 2048, 70), (100000, 100000, 65)])
def test_plan_covers_the_contracted_cloud(kind, n, m, t):
    from gpytorch_amd._lib import lib

    ldo = (n + 3) // 4 * 4
    rc, S, jc, ws = _plan(lib(), kind, n, m, 40, t, ldo)
    assert rc == 0 and S >= 1 and jc % 128 == 0 and S * jc >= m and (S - 1) * jc < m and ws > S * t * ldo


def test_refusals_without_gpu():
    from gpytorch_amd._lib import lib

    h = lib()
    for kind in (4, 8, -1):   # RQ, PP, nonsense
        assert _plan(h, kind, 10, 10, 40, 1, 12)[0] == -2 and b"Matern 1/2, 3/2, 5/2 only" in h.gpamd_last_error()
    for d in (32, 513):
        assert _plan(h, 1, 10, 10, d, 1, 12)[0] == -2 and b"33..512" in h.gpamd_last_error()
    for n, m, t, ldo in ((0, 10, 1, 12), (10, 0, 1, 12), (10, 10, 0, 12), (10, 10, 1, 8), (10, 10, 1, 14)):
        assert _plan(h, 1, n, m, 40, t, ldo)[0] == -1 and b"kv_wide_direct_plan: bad shape" in h.gpamd_last_error()

    def call(kind=1, x1=4096, n=1000, x2=4096, m=1000, d=40, dp=40, vt=4096, ldv=1000, t=11, p=4096, ldo=1000, S=1, jc=1024):
        # (the addresses are never read: every case below is refused before any launch)
        return h.gpamd_kv_wide_direct_partials_f32(kind, x1, n, x2, m, d, dp, vt, ldv, t, p, ldo, S, jc, None, None)

    assert call(kind=4) == -2 and b"Matern 1/2, 3/2, 5/2 only" in h.gpamd_last_error()
    assert call(d=32, dp=32) == -2 and call(d=513, dp=516) == -2 and b"33..512" in h.gpamd_last_error()
    for null in ("x1", "x2", "vt", "p"):
        assert call(**{null: None}) == -1 and b"null pointer" in h.gpamd_last_error()
    for bad in ({"n": 0}, {"t": 0}, {"S": 0}, {"dp": 36}, {"dp": 42}):
        assert call(**bad) == -1 and b"bad shape" in h.gpamd_last_error()
    for bad in ({"ldv": 996}, {"ldv": 1002}, {"ldo": 996}, {"ldo": 1002}):
        assert call(**bad) == -1 and b"leading dimensions" in h.gpamd_last_error()
    for ptr in ("x1", "x2", "vt", "p"):
        assert call(**{ptr: 4100}) == -1 and b"16-byte aligned" in h.gpamd_last_error()
    for bad in ({"jc": 1000}, {"jc": 896}, {"jc": 0}, {"S": 2, "jc": 384}):
        assert call(**bad) == -1 and b"jchunk % 128" in h.gpamd_last_error()
