"""The entry points of the wide direct-difference derivative (gpamd_kv_wide_direct_grad_*): the workspace count, and every refusal before any launch
-- no GPU needed."""
import pytest


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("n,m,d", [(77, 131, 33), (3000, 3000, 129), (640, 2048, 512), (100000, 100000, 40)])
def test_workspace_grows_with_the_columns(n, m, d, mode):
    from gpytorch_amd._lib import lib

    f = lib().gpamd_kv_wide_direct_grad_workspace_doubles
    counts = [f(n, m, d, t, mode) for t in (1, 11, 65, 66, 67, 133)]
    assert counts[0] > 0 and counts == sorted(counts) and counts[-1] > counts[0]
    assert f(n, m, 32, 11, mode) == 0 and f(n, m, 513, 11, mode) == 0 and f(0, m, d, 11, mode) == 0 and f(n, m, d, 0, mode) == 0 and f(n, m, d, 11, 2) == 0


def test_refusals_without_gpu():
    from gpytorch_amd._lib import lib

    h = lib()

    def call(kind=1, x1=4096, n=1000, x2=4096, m=1000, d=40, dp=40, lt=4096, ldl=1000, rt=4096, ldr=1000, t=11, mode=3, out=4096, gz=4096, ldg=40, ws=4096,
             nd=1 << 40):
        # (the addresses are never read: every case below is refused before any launch)
        return h.gpamd_kv_wide_direct_grad_f32(kind, x1, n, x2, m, d, dp, lt, ldl, rt, ldr, t, mode, out, gz, ldg, ws, nd, None)

    assert call(kind=4) == -2 and b"Matern 1/2, 3/2, 5/2 only" in h.gpamd_last_error()
    assert call(d=32, dp=32) == -2 and call(d=513, dp=516) == -2 and b"33..512" in h.gpamd_last_error()
    assert call(mode=2) == -1 and call(mode=4) == -1 and b"mode is 0" in h.gpamd_last_error()
    for null in ("x1", "x2", "lt", "rt", "out", "ws"):
        assert call(**{null: None}) == -1 and b"null pointer" in h.gpamd_last_error()
    assert call(gz=None) == -1 and call(ldg=39) == -1 and b"Gz1" in h.gpamd_last_error()
    assert call(gz=None, mode=1, nd=0) == -3   # (Gz1 is optional below mode 3: the call gets as far as the workspace)
    for bad in ({"n": 0}, {"m": 0}, {"t": 0}, {"dp": 36}, {"dp": 42}, {"ldl": 999}, {"ldr": 999}):
        assert call(**bad) == -1 and b"bad shape" in h.gpamd_last_error()
    for ptr in ("x1", "x2", "ws"):
        assert call(**{ptr: 4100}) == -1 and b"16-byte aligned" in h.gpamd_last_error()
    need = h.gpamd_kv_wide_direct_grad_workspace_doubles(1000, 1000, 40, 11, 3)
    assert call(nd=need - 1) == -3 and b"workspace too small" in h.gpamd_last_error()
