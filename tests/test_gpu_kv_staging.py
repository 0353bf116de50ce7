"""Tile staging of the fp32 K*V kernels (``csrc/kv_gram.hpp``, ``csrc/kv_mfma.hpp``): the full-tile fast path (every global load of a tile
issued back to back from one scalar base per row group and one per-thread 32-bit offset, rows c >= t clamped instead of branched around) moves data
only -- no arithmetic, no accumulation order -- so

  * every staging arm of ``libgpamd_tune.so`` (``csrc/tune/tune_stage.hip``) returns BITWISE the partial slabs of the parent's staging (arm 0), at the
    smallest shapes where staging can go wrong: a chunk of two full tiles plus a 60-row tail (m = 700), a tail that is no multiple of 4 (701), no
    tail (768), one partial tile shorter than a 32-row block (31), one full tile alone (128, S = 1), a partial last row block (n = 300) and n no
    multiple of 4 (257);
  * the product (``backend.kv``, fp32 contraction) stays within the K*V bound of tests/test_gpu_kv.py -- 2e-5 of max |oracle| against the float64
    oracle -- at shapes that take one row tile (CT = 1, NI = 4), the extra column, rows c >= t of the second column tile, d = 1, Matern-5/2 and,
    with max |z|^2 > 32, the direct-difference kernel."""
import ctypes as C
import os

import pytest
import torch

from oracle import kernels as OK
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = os.path.join(ROOT, "gpytorch_amd", "csrc", "libgpamd_tune.so")

# (variant, kind, d): the instantiations of tune_stage.hip, both t = 65 (CT = 2, NI = 2, EX = 1)
VARIANTS = [(0, "rbf", 3), (1, "matern52", 10)]
# (n, m, S, jchunk)
SHAPES = [(300, 700, 2, 384), (257, 701, 2, 384), (300, 768, 2, 384), (257, 31, 2, 384), (300, 128, 1, 384)]


def _stage_entry():
    h = C.CDLL(TUNE)
    if not hasattr(h, "gpamd_tune_stage_launch"):
        return None, 0
    f = h.gpamd_tune_stage_launch
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                  C.c_void_p]
    h.gpamd_tune_stage_arms.restype = C.c_int
    return f, int(h.gpamd_tune_stage_arms())


@pytest.mark.skipif(not os.path.exists(TUNE), reason="libgpamd_tune.so not built (make -C gpytorch_amd/csrc tune)")
@pytest.mark.parametrize("n,m,S,jc", SHAPES, ids=[f"n{s[0]}-m{s[1]}-S{s[2]}" for s in SHAPES])
@pytest.mark.parametrize("variant,kind,d", VARIANTS, ids=[f"{v[1]}-d{v[2]}" for v in VARIANTS])
def test_every_staging_arm_is_bitwise_the_parent_arm(variant, kind, d, n, m, S, jc, dev):
    from gpytorch_amd import backend as B

    f, arms = _stage_entry()
    assert f is not None, "libgpamd_tune.so has no gpamd_tune_stage_launch"
    new_arms = [s for s in range(1, 8) if arms >> s & 1]
    assert arms & 1 and new_arms, arms
    t = 65
    g = torch.Generator().manual_seed(1000 * variant + n + m)
    ls = 0.25 if d <= 3 else 0.8
    X1 = torch.rand(n, d, generator=g).to(dev)
    X2 = torch.rand(m, d, generator=g).to(dev)
    shift = X1.mean(0)
    p1, p2 = B.prep_points(kind, X1, torch.tensor(ls), shift), B.prep_points(kind, X2, torch.tensor(ls), shift)
    assert max(p1.zmax2, p2.zmax2) <= B.GRAM_MAX_SQNORM
    ldv, ldo = B.round_up(m, 4), B.round_up(n, 4)
    V = torch.randn(t, ldv, generator=g).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(stage):
        P = torch.zeros(S * t * ldo, device=dev)
        rc = f(variant, stage, p1.xp.data_ptr(), n, p2.xp.data_ptr(), m, V.data_ptr(), ldv, t, P.data_ptr(), ldo, S, jc, st)
        assert rc == 0, (stage, rc)
        torch.cuda.synchronize(dev)
        return P

    ref = run(0)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    for stage in new_arms:
        got = run(stage)
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero().reshape(-1)
            raise AssertionError(f"staging arm {stage}: {bad.numel()} of {ref.numel()} slab entries differ from the parent arm (first at {int(bad[0])})")


# (n, m, d, t, kind, lengthscale); lengthscale 0.02: max |z|^2 > 32 -> direct differences (kv_mfma.hpp)
PRODUCT = [
    (300, 31, 3, 65, "rbf", 0.44),
    (700, 1100, 3, 33, "rbf", 0.44),      # CT = 1, NI = 4, EX
    (1025, 1300, 2, 64, "rbf", 0.36),
    (600, 2100, 3, 40, "rbf", 0.44),      # rows c >= t of the second column tile
    (257, 128, 1, 64, "rbf", 0.28),
    (999, 3001, 3, 65, "matern52", 0.44),
    (600, 1100, 3, 65, "rbf", 0.02),      # max |z|^2 > 32
    (300, 500, 3, 70, "rbf", 0.44),       # CT = 3: twelve float4 of V per thread in chunks of eight -- the second chunk is short
    (300, 500, 3, 70, "rbf", 0.02),       # ... and on the direct-difference kernel
]


@pytest.mark.parametrize("n,m,d,t,kind,ls", PRODUCT, ids=[f"{c[4]}-n{c[0]}-m{c[1]}-d{c[2]}-t{c[3]}-ls{c[5]}" for c in PRODUCT])
def test_product_kv_f32_contraction_vs_float64_oracle(n, m, d, t, kind, ls, dev):
    from gpytorch_amd import backend as B

    g = torch.Generator().manual_seed(n + 7 * m + 13 * t)
    X1 = torch.rand(n, d, generator=g, dtype=torch.float64)
    X2 = torch.rand(m, d, generator=g, dtype=torch.float64)
    V = torch.randn(m, t, generator=g, dtype=torch.float64)
    # K(X1, X2) V as the first n rows of K(x, x) [0; V] on x = [X1; X2]
    ref = OK.kernel_matmul_rows(kind, torch.cat([X1, X2]), torch.arange(n), ls, 1.0, torch.cat([torch.zeros(n, t, dtype=torch.float64), V]))
    shift = X1.mean(0).float().to(dev)
    p1 = B.prep_points(kind, X1.float().to(dev), torch.as_tensor(ls), shift)
    p2 = B.prep_points(kind, X2.float().to(dev), torch.as_tensor(ls), shift)
    try:
        B.SPLIT_CONTRACTION = False
        flags = B.kv_flags(p1, p2, t)
        if ls < 0.1:
            assert max(p1.zmax2, p2.zmax2) > B.GRAM_MAX_SQNORM and flags == 0, (p1.zmax2, flags)
        else:
            assert flags == B.KV_GRAM, flags
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n)
    finally:
        B.SPLIT_CONTRACTION = None
    assert out.shape == (n, t)
    err = rel_err(out, ref)
    print(f"rel. error {err:.3e} (bound 2e-5)")
    assert err < 2e-5, err
