"""GPU: the W tile of the direct bilinear-derivative kernels (``kv_grad_tile``, csrc/kv_grad.hpp) where its skeleton can go wrong, once per kernel variant.

One shape for every family, n = 130, m = 600, t = 131:
  * n = 130: two rows in the first wave of the second block, whose other three waves are empty;
  * m = 600: two j chunks (320 + a 280-row tail: a partial 64-row step, a partial 32-column half);
  * t = 131: two column groups, the second of 3 columns (odd: the MFMA k-steps pad).
The families' existing derivative tests reach one column group and one j chunk only (t = 9, m <= 333).  Each case is compared with the float64
reference of that family's own test (tests/*_ref.py, dense autograd sums), in that test's error measure and with its bound; the inputs are drawn the
way that test draws them and the same preconditions are asserted.  One more case runs the single-family kernel on tile lists (far-pair culling) at
the smallest clouds ``far_cull`` accepts."""
import math

import pytest
import torch

from oracle import kernels as OK
from tests import test_gpu_additive as TA
from tests import test_gpu_far_cull as TF
from tests import test_gpu_gibbs as TG
from tests import test_gpu_newton_girard as TN
from tests import test_gpu_product as TP
from tests import test_gpu_sm as TS
from tests.additive_ref import add_terms
from tests.gibbs_ref import gibbs_grad_sums, gibbs_K, prefactor
from tests.newton_girard_ref import add_terms as ng_terms
from tests.newton_girard_ref import ng_grad_sums
from tests.piecewise_ref import pp_cov, pp_dist
from tests.product_ref import prod_cov
from tests import sm_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

N, M, T = 130, 600, 131


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


def _lr(gen, n=N, m=M, t=T):
    return torch.randn(n, t, generator=gen, dtype=torch.float64).float(), torch.randn(m, t, generator=gen, dtype=torch.float64).float()


def _direct(monkeypatch, B):
    """Keep ``hyper_grads`` on the direct-difference kernel and count its calls."""
    calls = []
    orig = B.kv_grad
    monkeypatch.setattr(B, "FORCE_GRAD_DIRECT", True)
    monkeypatch.setattr(B, "kv_grad", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


@pytest.mark.parametrize("ard", [False, True], ids=["iso", "ard"])
@pytest.mark.parametrize("kind", ["rbf", "matern12"])
def test_single_family(kind, ard, dev, monkeypatch):
    """kv_grad_kernel at dp = 4, one lengthscale and per-dimension: measure and bound of tests/test_gpu_model.py::test_kv_grad_kernel_ard_rectangular."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    d = 3
    gen = torch.Generator().manual_seed(40 + ard)
    X1, X2 = _f32(torch.rand(N, d, generator=gen, dtype=torch.float64)), _f32(torch.rand(M, d, generator=gen, dtype=torch.float64))
    Lm, Rm = _lr(gen)
    ls = _f32(0.3 + 0.2 * torch.rand(1, d if ard else 1, generator=gen, dtype=torch.float64)).requires_grad_(True)
    os_ = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    K = OK.kernel_matrix(kind, X1, X2, ls, os_, x1_eq_x2=False, direct=True)
    gl, go = torch.autograd.grad((Lm.double() * (K @ Rm.double())).sum(), [ls, os_])
    shift = None if kind == "rbf" else X1.mean(0).float().to(dev)
    lsd = ls.detach().float().to(dev)
    p1 = B.prep_points(kind, X1.float().to(dev), lsd, shift)
    p2 = B.prep_points(kind, X2.float().to(dev), lsd, shift)
    assert p1.dp == 4
    calls = _direct(monkeypatch, B)
    d_ls, d_os = hyper_grads(p1, p2, lsd, os_.detach().float().reshape(1).to(dev), B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
    assert len(calls) == 1
    e_ls, e_os = rel_err(d_ls, gl), abs(float(d_os) - float(go)) / abs(float(go))
    print("tile", kind, "ard" if ard else "iso", e_ls, e_os)
    assert e_ls < 1e-3 and e_os < 1e-3, (kind, ard, e_ls, e_os)


def test_piecewise_polynomial(dev, monkeypatch):
    """kv_grad_kernel<PP> (the shape code decoded before the tile loop), q = 1, per-dimension: measure and bound of
    tests/test_gpu_piecewise.py::test_backward_against_float64_autograd."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    d, q = 3, 1
    gen = torch.Generator().manual_seed(41)
    X1, X2 = _f32(torch.rand(N, d, generator=gen, dtype=torch.float64)), _f32(torch.rand(M, d, generator=gen, dtype=torch.float64))
    Lm, Rm = _lr(gen)
    ls = _f32(math.sqrt(d / 6.0) * (0.8 + 0.4 * torch.rand(1, d, generator=gen, dtype=torch.float64))).requires_grad_(True)
    os_ = torch.tensor(1.4, dtype=torch.float64, requires_grad=True)
    assert 0.05 < float((pp_dist(X1, X2, ls.detach()) < 1).double().mean()) < 0.95
    gl, go = torch.autograd.grad((Lm.double() * ((os_ * pp_cov(X1, X2, ls, q)) @ Rm.double())).sum(), [ls, os_])
    lsd = ls.detach().float().to(dev)
    shift = X1.mean(0).float().to(dev)
    p1 = B.prep_points("pp", X1.float().to(dev), lsd, shift, B.pp_code(d, q))
    p2 = B.prep_points("pp", X2.float().to(dev), lsd, shift, B.pp_code(d, q))
    calls = _direct(monkeypatch, B)
    d_ls, d_os = hyper_grads(p1, p2, lsd, torch.tensor([1.4], device=dev), B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
    assert len(calls) == 1 and B.far_cull(p1, p2) is None
    e_ls, e_os = rel_err(d_ls.reshape(-1), gl.reshape(-1)), rel_err(d_os.reshape(-1), go.reshape(-1))
    print("tile pp", e_ls, e_os)
    assert e_ls < 2e-3 and e_os < 2e-3, (e_ls, e_os)


def test_product_pair(dev):
    """kv_gradp_kernel, Matern-1/2 x Matern-5/2 with D_A = 1, D_B = 2: measure and bound of tests/test_gpu_product.py::test_bilinear_derivative."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    ka, kb, da, db = 1, 3, 1, 2
    gen = torch.Generator().manual_seed(42)
    X1, X2 = TP._cloud(gen, N, da + db), TP._cloud(gen, M, da + db)
    ls64 = TP._ls(gen, da + db).requires_grad_(True)
    os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    Lm, Rm = _lr(gen)
    K = prod_cov(ka, kb, da, X1, X2, ls64)
    TP._mixed(K.detach())
    g_ls, g_os = torch.autograd.grad((Lm.double() * ((os64 * K) @ Rm.double())).sum(), [ls64, os64])
    code, shift = B.prod_code(ka, kb, da), X1.mean(0)
    lsd = ls64.detach().float().to(dev).reshape(1, -1)
    p1, p2 = TP._prep(B, X1, ls64.detach(), shift, code, dev), TP._prep(B, X2, ls64.detach(), shift, code, dev)
    d_ls, d_os = hyper_grads(p1, p2, lsd, torch.tensor([1.3], device=dev), B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
    d_ls = d_ls.double().cpu().reshape(-1)
    e_ls = float((d_ls - g_ls).abs().max() / g_ls.abs().max())
    e_os = abs(float(d_os) - float(g_os)) / abs(float(g_os))
    print("tile prod", e_ls, e_os)
    assert e_ls < 2e-3 and e_os < 2e-3, (e_ls, e_os)


def test_additive(dev):
    """kv_grada_kernel over Matern-1/2, d = 3 (one NaN padding column), a lattice cloud against a uniform one: measure and bound of
    tests/test_gpu_additive.py::test_bilinear_derivative."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    kind, d = "matern12", 3
    gen = torch.Generator().manual_seed(43)
    X1, X2 = TA._lattice(gen, N, d), TA._cloud(gen, M, d)
    leaf = TA._ls(gen, d).requires_grad_(True)
    os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    Lm, Rm = _lr(gen)
    terms = add_terms(kind, X1, X2, leaf)
    TA._mixed(terms)
    g_ls, g_os = torch.autograd.grad((Lm.double() * ((os64 * terms.mean(-1)) @ Rm.double())).sum(), [leaf, os64])
    shift = X1.mean(0)
    lsd = leaf.detach().float().to(dev).reshape(1, -1)
    p1, p2 = TA._prep(B, X1, leaf.detach(), shift, kind, dev), TA._prep(B, X2, leaf.detach(), shift, kind, dev)
    assert p1.dp == 4 and bool(torch.isnan(p1.xp[:, d:]).all())
    d_ls, d_os = hyper_grads(p1, p2, lsd, torch.tensor([1.3], device=dev), B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
    d_ls = d_ls.double().cpu().reshape(-1)
    assert d_ls.numel() == d and bool(torch.isfinite(d_ls).all())
    e_ls = float((d_ls - g_ls.reshape(-1)).abs().max() / g_ls.abs().max())
    e_os = abs(float(d_os) - float(g_os)) / abs(float(g_os))
    print("tile add", e_ls, e_os)
    assert e_ls < 2e-3 and e_os < 2e-3, (e_ls, e_os)


def test_spectral_mixture(dev):
    """kv_grad_sm_kernel, Q = 2, d = 2: the sums, preconditions, measure and bound of tests/test_gpu_sm.py::test_derivative_sums_and_theta_gradients."""
    from gpytorch_amd import backend as B

    q, d = 2, 2
    gen = torch.Generator().manual_seed(44)
    X1, X2 = _f32(torch.rand(N, d, generator=gen, dtype=torch.float64)), _f32(torch.rand(M, d, generator=gen, dtype=torch.float64))
    w, mu, sigma = TS.sm_params(gen, q, d)
    Lm = (1.0 + 0.5 * torch.randn(N, T, generator=gen, dtype=torch.float64)).float()
    Rm = (1.0 + 0.5 * torch.randn(M, T, generator=gen, dtype=torch.float64)).float()
    TS._mixed(R.sm_cov(X1, X2, w, mu, sigma), w, d)
    g0, A, Bs, Cs, aA, aB, aC = R.sm_sums(X1, X2, w, mu, sigma, Lm.double() @ Rm.double().t())
    for name, v, av in (("A", A, aA), ("B", Bs, aB), ("C", Cs, aC)):
        assert float((v.abs() / av).min()) >= 1e-2, (name, v.abs() / av)
    shift = X1.mean(0)
    p1, p2 = TS._prep(B, X1, shift, w, mu, sigma, dev), TS._prep(B, X2, shift, w, mu, sigma, dev)
    g = B.kv_grad_sm(p1, p2, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))).double().cpu()
    ws, u = float(w.sum()), q * d
    what = (w / ws).reshape(q, 1)
    got = [g[0] * ws ** d, g[1 : 1 + u].reshape(q, d) * ws ** (d - 1) / what, g[1 + u : 1 + 2 * u].reshape(q, d) * ws ** d, g[1 + 2 * u :].reshape(q, d) * ws ** d]
    for name, a, b in zip(("k", "A", "B", "C"), got, (torch.tensor(g0), A, Bs, Cs)):
        e = float(((a - b).abs() / b.abs()).max())
        print("tile sm", name, e)
        assert e < 2e-3, (name, a, b)


def test_newton_girard(dev):
    """kv_grad_ng_kernel over Matern-5/2, d = 4, R = 4, lattice clouds: measure and bound of tests/test_gpu_newton_girard.py::test_bilinear_derivative_sums."""
    from gpytorch_amd import backend as B

    kind, d, r = "matern52", 4, 4
    gen = torch.Generator().manual_seed(45)
    X1, X2 = TN._cloud(gen, N, d, "lattice", kind), TN._cloud(gen, M, d, "lattice", kind)
    ls, sigma = TN._ls(gen, d), TN._sigma(gen, r)
    TN._check_cloud("lattice", ng_terms(kind, X1, X2, ls))
    Lm, Rm = _lr(gen)
    rc = B.ng_cap(d, r)
    ref = ng_grad_sums(kind, X1, X2, ls, sigma, Lm.double() @ Rm.double().t(), rc)
    shift = X1.mean(0)
    p1, p2 = TN._prep(B, X1, ls, shift, kind, sigma, dev), TN._prep(B, X2, ls, shift, kind, sigma, dev)
    got = B.kv_grad_ng(p1, p2, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))).double().cpu()
    assert got.shape == ref.shape == (1 + d + rc,) and bool(torch.isfinite(got).all())
    binom = torch.tensor([math.comb(d, k) for k in range(1, rc + 1)], dtype=torch.float64)
    e_k = abs(float(got[0] - ref[0])) / abs(float(ref[0]))
    e_q = float((got[1 : 1 + d] - ref[1 : 1 + d]).abs().max() / ref[1 : 1 + d].abs().max())
    e_e = float((((got[1 + d :] - ref[1 + d :]) / binom).abs().max()) / (ref[1 + d :] / binom).abs().max())
    print("tile ng", e_k, e_q, e_e)
    assert max(e_k, e_q, e_e) < 2e-3, (e_k, e_q, e_e)


@pytest.mark.parametrize("d", [2, 3], ids=["width4", "width8"])
def test_gibbs(d, dev):
    """kv_grad_gibbs_kernel at both prepared widths, the row side and (clouds and L, R exchanged: 600 rows against 130 columns) the column side; two
    runs give the same bits: measure and bound of tests/test_gpu_gibbs.py::test_derivative_pass."""
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(46 + d)
    X1, l1, X2, l2 = TG._cloud(gen, N, d), TG._ls(gen, N, d), TG._cloud(gen, M, d), TG._ls(gen, M, d)
    TG._mixed(gibbs_K(X1, l1, X2, l2), prefactor(l1, l2))
    Lm, Rm = _lr(gen)
    g0, g1, g2 = gibbs_grad_sums(X1, l1, X2, l2, Lm.double() @ Rm.double().t())
    shift = X1.mean(0)
    p1, p2 = TG._prep(B, X1, l1, shift, dev), TG._prep(B, X2, l2, shift, dev)
    assert p1.dp == (4 if d <= 2 else 8)
    lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
    G0, r1 = B.kv_grad_gibbs(p1, p2, lt, rt)
    H0, r2 = B.kv_grad_gibbs(p2, p1, rt, lt)
    assert r1.shape == (N,) and r2.shape == (M,) and bool(torch.isfinite(r1).all()) and bool(torch.isfinite(r2).all())
    G0b, r1b = B.kv_grad_gibbs(p1, p2, lt, rt)
    assert torch.equal(G0, G0b) and torch.equal(r1, r1b)                          # no atomics: the same bits
    e_0 = max(abs(float(G0) - float(g0)), abs(float(H0) - float(g0))) / abs(float(g0))
    e_1 = float((r1.double().cpu() - g1).abs().max() / g1.abs().max())
    e_2 = float((r2.double().cpu() - g2).abs().max() / g2.abs().max())
    print("tile gibbs", d, e_0, e_1, e_2)
    assert max(e_0, e_1, e_2) < 2e-3, (d, e_0, e_1, e_2)


def test_single_family_on_tile_lists(dev):
    """kv_grad_kernel<Matern-5/2> walking tile lists, n = m = ``FAR_MIN_POINTS`` (the smallest clouds ``far_cull`` accepts), two column
    groups on one list.  Some steps drop out and some remain, read off the lists themselves; culled against un-culled in the measure
    and bound of tests/test_gpu_far_cull.py::test_bilinear_derivative_is_culled_too (vectors of one sign, 2e-5 of the largest sum), and both against the
    dense float64 sums within the 1e-3 of tests/test_gpu_model.py::test_kv_grad_kernel_ard_rectangular."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    kind, ls = "matern52", 0.02
    n = B.FAR_MIN_POINTS
    # points along one smooth curve, a hundred lengthscales long: its eight 128-point chunks are compact next to their distances (the 40 short roads of
    # tests/test_gpu_far_cull.py::road_like leave, at 1024 points, chunks whose spheres all overlap: nothing drops at any lengthscale)
    gen = torch.Generator().manual_seed(9)
    u = torch.rand(n, generator=gen)
    X = torch.stack([u, 0.3 * torch.sin(6 * u), 0.3 * torch.cos(4 * u)], -1) + 0.002 * torch.randn(n, 3, generator=gen)
    xp = TF._prep(B, kind, X, ls, dev)
    gen = torch.Generator().manual_seed(T)
    Lm, Rm = torch.rand(n, T, generator=gen) + 0.1, torch.rand(n, T, generator=gen) + 0.1
    lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
    g0 = B.kv_grad(xp, xp, lt, rt, iso=True)
    with g.settings.far_pair_cutoff(1e-7):
        assert B.far_cull(xp, xp) is not None
        g1 = B.kv_grad(xp, xp, lt, rt, iso=True)
        # every unit's list as the list kernel left it: ascending step starts, then the terminator (= the end of the unit's j chunk).  Unit 0's
        # terminator is the chunk length (tests/test_gpu_far_cull.py reads it the same way)
        tl = B._far_ws[lt.device][: int(B.lib().gpamd_kv_grad_far_workspace_ints(n, n))].tolist()
    k = 1
    while k < len(tl) and tl[k] > tl[k - 1]:
        k += 1
    chunk = tl[k - 1]
    assert chunk % 64 == 0 and 0 < chunk <= B.round_up(n, 64)
    tpc1, nrb, S = chunk // 64 + 1, (n + 127) // 128, (n + chunk - 1) // chunk
    assert len(tl) == nrb * S * tpc1
    kept = total = 0
    for unit in range(nrb * S):
        s, lst = unit // nrb, tl[unit * tpc1 : (unit + 1) * tpc1]
        steps = lst[: lst.index((s + 1) * chunk)]
        assert steps == sorted(set(steps)) and all(s * chunk <= j < min(n, (s + 1) * chunk) and j % 64 == 0 for j in steps)
        kept += len(steps)
        total += (min(n, (s + 1) * chunk) - s * chunk + 63) // 64
    print("tile lists: kept", kept, "of", total)
    assert 0 < kept < total, (kept, total)
    sc = float(g0.abs().max())
    assert float((g1 - g0).abs().max()) < 2e-5 * sc, (g0.tolist(), g1.tolist())
    X64 = X.double()
    lsr = torch.tensor([[ls]], dtype=torch.float64, requires_grad=True)
    os_ = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    K = OK.kernel_matrix(kind, X64, X64, lsr, os_, x1_eq_x2=False, direct=True)
    gl, go = torch.autograd.grad((Lm.double() * (K @ Rm.double())).sum(), [lsr, os_])
    for name, gg in (("un-culled", g0), ("culled", g1)):
        gg = gg.double().cpu()
        d_ls = -2.0 / ls * gg[1 : 1 + xp.d].sum()                             # functions.hyper_grads for one lengthscale, outputscale 1
        e_ls, e_os = abs(float(d_ls) - float(gl)) / abs(float(gl)), abs(float(gg[0]) - float(go)) / abs(float(go))
        print("tile lists", name, e_ls, e_os)
        assert e_ls < 1e-3 and e_os < 1e-3, (name, e_ls, e_os)
