"""GPU: the piecewise-polynomial covariance family (``kernels.PiecewisePolynomialKernel``, ``KIND_PP``) and its EXACT tile culling
(``settings.compact_support_culling``).

Oracle: tests/piecewise_ref.py, the float64 restatement that tests/test_piecewise_cpu.py pins to outputs of the reference's own code
(tests/golden/piecewise_values.npz).  Tolerances are those of the RQ family's tests (tests/test_gpu_kv.py, tests/test_gpu_compose.py):
4e-6 on entries of K, 5e-5 max |K V| on products, the RQ model test's bounds for the marginal log likelihood and its gradients.

Input gradients for q = 0 do not exist (a cusp at r = 0: refused loudly, as for Matern nu = 1/2 outside the Gram policy)."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import exact_gp as OG
from oracle import kernels as OK
from tests.piecewise_ref import pp_cov, pp_dist
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "piecewise_values.npz")


def _prep(B, X, ls, q, dev, shift=True, dtype=torch.float32):
    Xd = X.to(device=dev, dtype=dtype)
    return B.prep_points("pp", Xd, torch.as_tensor(ls), Xd.mean(0) if shift else None, B.pp_code(X.shape[1], q))


def _ref_rows(X, rows, ls, q, V, dev, chunk=256):
    """Rows ``rows`` of pp_cov(X, X) @ V in float64, formed on the device a few hundred rows at a time."""
    X64, V64 = X.to(device=dev, dtype=torch.float64), V.to(device=dev, dtype=torch.float64)
    ls64 = torch.as_tensor(ls, dtype=torch.float64, device=dev)
    out = [pp_cov(X64[rows[r0 : r0 + chunk]], X64, ls64, q) @ V64 for r0 in range(0, rows.numel(), chunk)]
    return torch.cat(out, 0).cpu()


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_dense_rows_diag_every_q(q, dev):
    from gpytorch_amd import backend as B

    n, m = 130, 77
    for d in (1, 3, 10, 16):
        for ard in (False, True):
            g = torch.Generator().manual_seed(100 * d + q)
            X1 = torch.rand(n, d, generator=g, dtype=torch.float64).float().double()     # (what the float32 kernels receive, exactly)
            X2 = torch.rand(m, d, generator=g, dtype=torch.float64).float().double()
            ls = math.sqrt(d / 6.0) * (0.8 + 0.4 * torch.rand(d if ard else 1, generator=g, dtype=torch.float64)).float().double()
            shift = X1.mean(0).float().to(dev)
            code = B.pp_code(d, q)
            p1 = B.prep_points("pp", X1.float().to(dev), ls, shift, code)
            p2 = B.prep_points("pp", X2.float().to(dev), ls, shift, code)
            scale = torch.tensor([1.7], device=dev)
            Kref = 1.7 * pp_cov(X1, X2, ls, q)
            r = pp_dist(X1, X2, ls)
            assert 0.05 < float((r < 1).double().mean()) < 0.95, (d, ard)
            K = B.kernel_dense(p1, p2, scale).double().cpu()
            err = float((K - Kref).abs().max())
            print("dense", q, d, ard, err)
            assert err < 4e-6, (q, d, ard, err)
            assert bool((K[r >= 1 + 1e-3] == 0).all()), "exact zeros outside the support"
            rows = torch.tensor([0, n - 1, n // 2])
            assert float((B.kernel_rows(p1, rows, p2, scale).double().cpu() - Kref[rows]).abs().max()) < 4e-6
            q1 = B.prep_points("pp", X1[:m].float().to(dev), ls, shift, code)
            assert float((B.kernel_diag(q1, p2, scale).double().cpu() - Kref[:m].diagonal()).abs().max()) < 4e-6
            assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n))               # x1 is x2: exact unit diagonal
            assert torch.equal(B.kernel_dense(p1, p1).diagonal().cpu(), torch.ones(n))
            # float64 generation (the generic path): 1e-12, as tests/test_gpu_generic.py holds the other families to
            d1 = B.prep_points("pp", X1.to(dev), ls, shift.double(), code)
            d2 = B.prep_points("pp", X2.to(dev), ls, shift.double(), code)
            K64 = B.kernel_dense(d1, d2).cpu()
            assert K64.dtype == torch.float64 and float((K64 - Kref / 1.7).abs().max()) < 1e-12
            assert bool((K64[r >= 1 + 1e-3] == 0).all())


def test_kernel_class_against_reference_generated_fixtures(dev):
    """``PiecewisePolynomialKernel(q)(x1, x2).to_dense()`` against outputs of the reference's own forward: 4e-6 for the float64 fixtures; for the
    float32 ones the rule of tests/test_gpu_kv.py::test_golden_kernel_values (the reference's Gram-trick distance in float32: 5e-5, and 3e-4 where k
    has a cusp at r = 0 -- there Matern nu = 1/2, here q = 0)."""
    import gpytorch_amd as g

    z = np.load(GOLDEN)
    for name in "abcdefgh":
        x1, x2, ls = (torch.from_numpy(z[f"{name}_{k}"]) for k in ("x1", "x2", "ls"))
        f32 = z[f"{name}_x1"].dtype == np.float32
        same = bool(z[f"{name}_same"])
        for q in range(4):
            kern = g.kernels.PiecewisePolynomialKernel(q=q, ard_num_dims=x1.shape[1] if ls.numel() > 1 else None).to(dev)
            kern.lengthscale = ls.float()
            xa = x1.float().to(dev)
            K = kern(xa, xa if same else x2.float().to(dev)).to_dense().double().cpu()
            err = float((K.detach() - torch.from_numpy(z[f"{name}_K{q}"]).double()).abs().max())
            print("golden", name, q, err)
            assert err < ((3e-4 if q == 0 else 5e-5) if f32 else 4e-6), (name, q, err)


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_kv_on_every_dispatch_route(q, dev):
    """One shape per route, as the non-RBF families are swept in tests/test_gpu_kv.py::test_kv_matches_oracle: direct differences on the VALU / fp32 MFMA
    kernels, the Gram form at 1-2 columns (kv_gramv), in 4-column groups (kv_gram4), 16- and 32-column tiles, the split contraction on the Gram form
    (kv_gramh) and on direct differences (kv_directh).  q = 0 has a cusp at r = 0 and keeps to the direct-difference routes."""
    from gpytorch_amd import backend as B

    shapes = [(300, 300, 3, 1), (411, 300, 2, 2), (513, 700, 3, 4), (777, 1000, 3, 11), (640, 900, 6, 16), (257, 300, 3, 32), (700, 1100, 3, 33),
              (600, 2100, 3, 65), (520, 640, 10, 128)]
    for n, m, d, t in shapes:
        g = torch.Generator().manual_seed(n + 7 * m + 13 * t)
        X1 = torch.rand(n, d, generator=g, dtype=torch.float64).float()
        X2 = torch.rand(m, d, generator=g, dtype=torch.float64).float()
        V = torch.randn(m, t, generator=g, dtype=torch.float64)
        ls = 0.2 + 0.08 * d
        code = B.pp_code(d, q)
        shift = X1.mean(0).to(dev)
        p1 = B.prep_points("pp", X1.to(dev), torch.tensor([ls]), shift, code)
        p2 = B.prep_points("pp", X2.to(dev), torch.tensor([ls]), shift, code)
        vt = B.to_probe_major(V.to(dev))
        ref = pp_cov(X1.double(), X2.double(), torch.tensor([ls]), q) @ V
        assert max(p1.zmax2, p2.zmax2) <= B.GRAM_MAX_SQNORM
        flag_sets = [0, B.KV_SPLIT] if q == 0 else [0, B.KV_SPLIT, B.KV_GRAM, B.KV_GRAM | B.KV_G4, B.KV_GRAM | B.KV_WIDE, B.KV_GRAM | B.KV_SPLIT]
        try:
            for flags in flag_sets:
                if (flags & B.KV_SPLIT) and not (flags & B.KV_GRAM) and d > B.DIRECT_SPLIT_MAX_DIM:
                    continue
                B.FORCE_KV_FLAGS = flags
                err = rel_err(B.from_probe_major(B.kv(p1, p2, vt), n), ref)
                print("kv", q, (n, m, d, t), flags, err)
                assert err < 5e-5, (q, n, m, d, t, flags, err)
        finally:
            B.FORCE_KV_FLAGS = None
        # the automatic policy, both contractions
        for split in (True, False):
            B.SPLIT_CONTRACTION = split
            try:
                assert bool(B.kv_flags(p1, p2, t) & B.KV_GRAM) == (q != 0)
                err = rel_err(B.from_probe_major(B.kv(p1, p2, vt), n), ref)
                assert err < 5e-5, (q, n, m, d, t, "auto", split, err)
            finally:
                B.SPLIT_CONTRACTION = None


@pytest.mark.parametrize("q", [0, 2])
def test_kv_float64_and_twenty_dimensions(q, dev):
    """float64 clouds (fused float64 kernel for d <= 16, dense row blocks x GEMM otherwise) and d = 20: on the fused float32 kernels and through the
    generic path (``FORCE_GENERIC``)."""
    from gpytorch_amd import backend as B

    g = torch.Generator().manual_seed(q)
    for d, dtype, force in [(3, torch.float64, False), (20, torch.float64, False), (20, torch.float32, False), (20, torch.float32, True)]:
        n, m, t = 700, 900, 9
        X1 = torch.rand(n, d, generator=g, dtype=torch.float64).float().double()
        X2 = torch.rand(m, d, generator=g, dtype=torch.float64).float().double()
        V = torch.randn(m, t, generator=g, dtype=torch.float64)
        ls = torch.tensor([math.sqrt(d / 6.0)])
        ref = pp_cov(X1, X2, ls, q) @ V
        code = B.pp_code(d, q)
        sh = X1.mean(0).to(device=dev, dtype=dtype)
        try:
            B.FORCE_GENERIC = force
            p1 = B.prep_points("pp", X1.to(device=dev, dtype=dtype), ls, sh, code)
            p2 = B.prep_points("pp", X2.to(device=dev, dtype=dtype), ls, sh, code)
            assert p1.fused == (dtype == torch.float32 and not force)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev), dtype)), n)
        finally:
            B.FORCE_GENERIC = False
        err = rel_err(out, ref)
        print("kv generic", q, d, dtype, force, err)
        assert err < (1e-12 if dtype == torch.float64 else 5e-5), (q, d, dtype, force, err)


def test_culling_is_exact(dev):
    """n = 65 536 uniform points in the unit square, lengthscale 0.02: the products with the culling on (the default) and off agree with float64 rows of
    the restatement and with each other at the K V tolerance, fewer than a quarter of the (row block, tile) pairs survive, and the culled entry point
    is the one that ran."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    n, ls, q = 65536, 0.02, 2
    gen = torch.Generator().manual_seed(11)
    X = torch.rand(n, 2, generator=gen)
    rows = torch.randperm(n, generator=gen)[:2048]
    xp = _prep(B, X, [ls], q, dev)
    assert g.settings.far_pair_cutoff.value() is None and B.far_cull(xp, xp) == 1.0
    kept = B.far_kept_fraction(xp, xp, 1.0)
    print("kept fraction of (512-row block, tile) pairs:", kept)
    assert kept < 0.25, kept
    launches = []
    orig = B._kv_launch

    def spy(*a):
        launches.append(a[15] is not None)     # the `cull` argument
        return orig(*a)

    B._kv_launch = spy
    try:
        for t in (1, 11, 65):
            V = torch.randn(n, t, generator=gen)
            vt = B.to_probe_major(V.to(dev))
            ref = _ref_rows(X, rows, [ls], q, V, dev)
            del launches[:]
            plan = B.KvPlan(xp, xp, t)
            assert plan.rows_sorted
            if t < 5:
                assert plan.flags & B.KV_SPLIT_FEW     # few enough tiles survive: the few-column product moves to the culled split kernels
            on = B.from_probe_major(B.kv(xp, xp, vt), n).cpu()
            assert launches and all(launches), "the culled entry point was not taken"
            del launches[:]
            with g.settings.compact_support_culling(False):
                assert B.far_cull(xp, xp) is None
                off = B.from_probe_major(B.kv(xp, xp, vt), n).cpu()
            assert launches and not any(launches)
            e_on, e_off, e_both = rel_err(on[rows], ref), rel_err(off[rows], ref), rel_err(on, off)
            print("culling t =", t, "on", e_on, "off", e_off, "on vs off", e_both)
            assert e_on < 5e-5 and e_off < 5e-5 and e_both < 5e-5, (t, e_on, e_off, e_both)
    finally:
        B._kv_launch = orig


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_backward_against_float64_autograd(q, ard, dev):
    """Lengthscale (one / ARD), outputscale and input gradients of a product's squared norm, culled and un-culled, against float64 autograd of the
    restatement; bounds of tests/test_gpu_compose.py::test_rq_kernel_values_products_and_all_gradients.  q >= 1: the Gram-form derivative kernel
    (block-centred, walking the tile lists when culled); q = 0: the direct-difference derivative kernel (``gpamd_kv_grad_param_far_f32``, on tile lists when
    culled), hyper-parameters only."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    n, d, t = 4096, 2, 9
    gen = torch.Generator().manual_seed(5 + q)
    X = torch.rand(n, d, generator=gen)
    V = torch.randn(n, t, generator=gen)
    ls = torch.tensor([[0.05, 0.07]]) if ard else torch.tensor([[0.06]])
    want_x = q != 0
    # float64 autograd on the device
    ls64 = ls.double().to(dev).requires_grad_(True)
    os64 = torch.tensor(1.4, dtype=torch.float64, device=dev, requires_grad=True)
    x64 = X.double().to(dev).requires_grad_(True)
    (os64 * pp_cov(x64, x64, ls64, q) @ V.double().to(dev)).pow(2).sum().backward()
    sig = lambda raw: torch.sigmoid(raw.detach().double())  # noqa: E731
    for cull in (True, False):
        kern = g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=q, ard_num_dims=d if ard else None)).to(dev)
        kern.base_kernel.lengthscale = ls
        kern.outputscale = 1.4
        xa = X.to(dev).requires_grad_(want_x)
        seen = []
        orig = B.far_cull
        B.far_cull = lambda a, b: (seen.append(orig(a, b)), seen[-1])[1]
        try:
            with warnings.catch_warnings(), g.settings.compact_support_culling(cull):
                warnings.simplefilter("ignore")
                (kern(xa, xa) @ V.to(dev)).pow(2).sum().backward()
        finally:
            B.far_cull = orig
        assert seen and all((s == 1.0) if cull else (s is None) for s in seen), (cull, seen)
        bk = kern.base_kernel
        e_ls = rel_err(bk.raw_lengthscale.grad.reshape(-1), (ls64.grad * sig(bk.raw_lengthscale)).reshape(-1))
        e_os = rel_err(kern.raw_outputscale.grad.reshape(-1), (os64.grad * sig(kern.raw_outputscale)).reshape(-1))
        print("backward", q, ard, cull, "ls", e_ls, "os", e_os)
        assert e_ls < 2e-3 and e_os < 2e-3, (q, ard, cull, e_ls, e_os)
        if want_x:
            e_x = rel_err(xa.grad, x64.grad)
            print("backward", q, ard, cull, "x", e_x)
            assert e_x < 2e-3, (q, ard, cull, e_x)
    if q == 0:
        xa = X.to(dev).requires_grad_(True)
        with pytest.raises(RuntimeError, match="gradients with respect to the inputs"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            (kern(xa, xa) @ V.to(dev)).pow(2).sum().backward()


@pytest.mark.parametrize("q", [0, 1, 2])
def test_backward_on_a_cloud_with_a_sparse_tail(q, dev):
    """A dense cluster plus a sparse tail: the 128-point runs of the tail are wider than the quadratic expansion's policy (``sorted_view().n_block < n``),
    so the Gram-form derivative kernel sees the compact rows only and the WIDE rows take the direct-difference derivative kernel -- through the entry
    point that carries the family's shape code, walking tile lists when culled -- or, with input gradients, the row-block derivative.  q = 0 runs on the
    direct-difference derivative kernel as a whole.  Culled and un-culled against float64 autograd of the restatement; bounds of
    test_backward_against_float64_autograd."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B

    n, d, t, ls = 8192, 2, 9, 0.06
    gen = torch.Generator().manual_seed(21 + q)
    X = torch.cat([torch.rand(n - 1024, d, generator=gen), 40.0 * torch.rand(1024, d, generator=gen) - 20.0])[torch.randperm(n, generator=gen)]
    V = torch.randn(n, t, generator=gen)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xp = _prep(B, X, [ls], q, dev)
        assert B.gram_mode(xp, xp) == 2 and xp.sorted_view().n_block < n, "the cloud must have wide rows"
    ls64 = torch.tensor([[ls]], dtype=torch.float64, device=dev, requires_grad=True)
    os64 = torch.tensor(1.4, dtype=torch.float64, device=dev, requires_grad=True)
    x64 = X.double().to(dev).requires_grad_(True)
    (os64 * pp_cov(x64, x64, ls64, q) @ V.double().to(dev)).pow(2).sum().backward()
    sig = lambda raw: torch.sigmoid(raw.detach().double())  # noqa: E731
    for cull in (True, False):
        for want_x in ((False, True) if q else (False,)):
            kern = g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=q)).to(dev)
            kern.base_kernel.lengthscale = ls
            kern.outputscale = 1.4
            xa = X.to(dev).requires_grad_(want_x)
            seen, direct = [], []
            orig_cull, orig_grad = B.far_cull, B.kv_grad
            B.far_cull = lambda a, b: (seen.append(orig_cull(a, b)), seen[-1])[1]
            B.kv_grad = lambda *a, **kw: (direct.append(kw.get("far") is not None or orig_cull(a[0], a[1]) is not None), orig_grad(*a, **kw))[1]
            try:
                with warnings.catch_warnings(), g.settings.compact_support_culling(cull):
                    warnings.simplefilter("ignore")
                    (kern(xa, xa) @ V.to(dev)).pow(2).sum().backward()
            finally:
                B.far_cull, B.kv_grad = orig_cull, orig_grad
            assert seen and all((s_ == 1.0) if cull else (s_ is None) for s_ in seen), (cull, seen)
            if not want_x:   # the direct-difference derivative kernel ran (wide rows; everything for q = 0), on tile lists exactly when culled
                assert direct and all(c == cull for c in direct), (q, cull, direct)
            bk = kern.base_kernel
            e_ls = rel_err(bk.raw_lengthscale.grad.reshape(-1), (ls64.grad * sig(bk.raw_lengthscale)).reshape(-1))
            e_os = rel_err(kern.raw_outputscale.grad.reshape(-1), (os64.grad * sig(kern.raw_outputscale)).reshape(-1))
            print("tail backward", q, cull, want_x, "ls", e_ls, "os", e_os)
            assert e_ls < 2e-3 and e_os < 2e-3, (q, cull, want_x, e_ls, e_os)
            if want_x:
                e_x = rel_err(xa.grad, x64.grad)
                print("tail backward", q, cull, "x", e_x)
                assert e_x < 2e-3, (q, cull, e_x)


def _gp_class(g, make_kernel, mean=None):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean() if mean is None else mean()
            self.covar_module = make_kernel()

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_gp_mll_cholesky_and_bbmm(q, dev):
    """ScaleKernel(PiecewisePolynomialKernel(q)) ExactGP, n = 3000, d = 2: the marginal log likelihood and its gradients on the Cholesky branch and
    on the BBMM branch (deterministic probes) against dense float64 autograd; bounds of tests/test_gpu_compose.py::test_rq_gp_mll_bbmm_and_cholesky.
    The BBMM branch runs with 100 Lanczos quadrature nodes: the log determinant's Gauss quadrature at the default 20 nodes, without a preconditioner,
    is biased by 0.3e-2 .. 2.4e-2 of the value at n = 3000 for EVERY family (measured on the same data: Matern-1/2 2.4e-2, Matern-5/2 6.5e-3,
    this family 3.4e-3 .. 1.1e-2, unchanged by ten times the probes), and by 0.2e-4 .. 6e-4 at 100 -- an estimator setting, not the bound
    (scripts/pp_estimator_settings.py -> profiles/pp_estimator_settings.json)."""
    import gpytorch_amd as g

    n, d = 3000, 2
    X, y = make_data(n, d)
    X, y = X.float().double(), y.float().double()
    p = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.3, 1.3, 0.1)]   # lengthscale, outputscale, noise
    ref = OG.dense_log_prob(p[1] * pp_cov(X, X, p[0].reshape(1), q) + p[2] * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, p)
    M = _gp_class(g, lambda: g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=q)))
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        m.covar_module.base_kernel.lengthscale = 0.3
        m.covar_module.outputscale = 1.3
        lik.noise = 0.1
        mll = g.ExactMarginalLogLikelihood(lik, m)
        m.train()
        lik.train()
        S = g.settings
        with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(300), \
                S.max_preconditioner_size(0), S.deterministic_probes(True), S.max_lanczos_quadrature_iterations(100):
            warnings.simplefilter("ignore")
            torch.manual_seed(0)
            val = mll(m(m.train_inputs[0]), m.train_targets)
            val.backward()
            S.deterministic_probes.reset()
        tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
        sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731
        got = torch.tensor([float(m.covar_module.base_kernel.raw_lengthscale.grad.sum()), float(m.covar_module.raw_outputscale.grad),
                            float(lik.noise_covar.raw_noise.grad.sum())], dtype=torch.float64)
        want = torch.tensor([float(gref[0]) * sp(0.3), float(gref[1]) * sp(1.3), float(gref[2]) * sp(0.1 - 1e-4)], dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("mll", q, branch, e_v, e_g)
        assert e_v < tol_v, (q, branch, float(val), float(ref))
        assert e_g < tol_g, (q, branch, got, want)
        assert sorted(k for k, _ in m.covar_module.base_kernel.named_parameters()) == ["raw_lengthscale"]


def test_gp_posterior_fast_pred_var(dev):
    """Posterior mean and variance of the same model (q = 2) against the dense float64 posterior: with ``fast_pred_var`` (LOVE) and with the exact
    variance.  LOVE is a rank-r approximation of the variance from above whose error follows the spectrum of K, and this family's eigenvalues decay
    polynomially: on this data the error is 3.6 of the variance at the default r = 100, 0.10 at 400, 8e-4 at 1500 (Matern-5/2: 1.3e-2 at 100, 1.5e-5
    at 400), so the cache is built with r = 1500.  Bounds: the mean and the exact variance as tests/test_gpu_far_cull.py holds a posterior mean whose
    solves stop at eval_cg_tolerance = 1e-4 (2e-3); the LOVE variance at the reference's own bound for fast_pred_var, 5 %
    (test/examples/test_simple_gp_regression.py:396-442).  The measurements: scripts/pp_estimator_settings.py -> profiles/pp_estimator_settings.json."""
    import gpytorch_amd as g

    n, ns, d, q = 3000, 200, 2, 2
    X, y = make_data(n + ns, d)
    X, y = X.float().double(), y.float().double()
    Xt, yt, Xs = X[:n], y[:n], X[n:]
    ls = torch.tensor([0.3], dtype=torch.float64)
    Lc = torch.linalg.cholesky(1.3 * pp_cov(Xt, Xt, ls, q) + 0.1 * torch.eye(n, dtype=torch.float64))
    Ks = 1.3 * pp_cov(Xs, Xt, ls, q)
    mu_ref = (Ks @ torch.cholesky_solve(yt.unsqueeze(-1), Lc)).squeeze(-1)
    var_ref = 1.3 + 0.1 - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)
    M = _gp_class(g, lambda: g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=q)))
    S = g.settings
    for fast in (True, False):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(Xt.float().to(dev), yt.float().to(dev), lik).to(dev)
        m.covar_module.base_kernel.lengthscale, m.covar_module.outputscale, lik.noise = 0.3, 1.3, 0.1
        m.eval()
        lik.eval()
        torch.manual_seed(1)
        with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4), \
                S.max_root_decomposition_size(1500):
            warnings.simplefilter("ignore")
            pred = lik(m(Xs.float().to(dev)))
            mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
        e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
        print("posterior fast_pred_var", fast, e_mu, e_var)
        assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)


def test_batch_of_small_members_and_additive_kernel(dev):
    """Three small members through the stacked evaluation (gpytorch_amd/batched.py) == the member loop == dense float64; and
    AdditiveKernel(ScaleKernel(RBF), ScaleKernel(PP)) against the dense sum."""
    import gpytorch_amd as g
    from gpytorch_amd import batched

    b, n, d, q = 3, 150, 3, 2
    gen = torch.Generator().manual_seed(3)
    X = torch.rand(b, n, d, generator=gen)
    Y = torch.sin(3 * X.sum(-1)) + 0.1 * torch.randn(b, n, generator=gen)
    bs = torch.Size([b])
    ls = 0.5 + 0.5 * torch.rand(b, 1, 1, generator=gen)
    os_ = 0.7 + torch.rand(b, generator=gen)
    nz = 0.05 + 0.2 * torch.rand(b, 1, generator=gen)
    M = _gp_class(g, lambda: g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=q, batch_shape=bs), batch_shape=bs))

    def evaluate(stacked):
        lik = g.likelihoods.GaussianLikelihood(batch_shape=bs).to(dev)
        m = M(X.to(dev), Y.to(dev), lik).to(dev)
        m.covar_module.base_kernel.lengthscale, m.covar_module.outputscale, lik.noise = ls, os_, nz
        mll = g.ExactMarginalLogLikelihood(lik, m)
        m.train()
        lik.train()
        calls = []
        orig = batched.BatchedCholeskyInvQuadLogdetFn.apply
        batched.BatchedCholeskyInvQuadLogdetFn.apply = lambda *a: (calls.append(1), orig(*a))[1]
        try:
            with g.settings.batched_small_members(stacked):
                val = mll(m(m.train_inputs[0]), m.train_targets)
                val.sum().backward()
        finally:
            batched.BatchedCholeskyInvQuadLogdetFn.apply = orig
        assert len(calls) == (1 if stacked else 0)
        grads = [m.covar_module.base_kernel.raw_lengthscale.grad, m.covar_module.raw_outputscale.grad, lik.noise_covar.raw_noise.grad]
        return val.detach().double().cpu(), [x.detach().double().cpu().reshape(b, -1) for x in grads]

    v1, g1 = evaluate(True)
    v0, g0 = evaluate(False)
    assert torch.allclose(v1, v0, rtol=2e-5, atol=2e-5)
    for a, c in zip(g1, g0):
        assert torch.allclose(a, c, rtol=3e-3, atol=3e-3 * float(c.abs().max())), (a, c)
    for i in range(b):
        Kh = os_[i].double() * pp_cov(X[i].double(), X[i].double(), ls[i].double().reshape(1), q) + nz[i].double() * torch.eye(n, dtype=torch.float64)
        assert abs(float(v1[i]) - float(OG.dense_log_prob(Kh, Y[i].double()) / n)) < 2e-4

    # AdditiveKernel(RBF, PP): dense values, a product and the MLL on the Cholesky branch
    n2 = 900
    X2, y2 = make_data(n2, 2)
    X2, y2 = X2.float().double(), y2.float().double()
    kern = (g.kernels.ScaleKernel(g.kernels.RBFKernel()) + g.kernels.ScaleKernel(g.kernels.PiecewisePolynomialKernel(q=1))).to(dev)
    kern.kernels[0].base_kernel.lengthscale, kern.kernels[0].outputscale = 0.4, 0.8
    kern.kernels[1].base_kernel.lengthscale, kern.kernels[1].outputscale = 0.25, 1.2
    Kref = 0.8 * OK.rbf(X2, X2, 0.4, direct=True) + 1.2 * pp_cov(X2, X2, torch.tensor([0.25]), 1)
    xd = X2.float().to(dev)
    assert rel_err(kern(xd, xd).to_dense(), Kref) < 1e-5
    V = torch.randn(n2, 7, generator=gen)
    assert rel_err(kern(xd, xd) @ V.to(dev), Kref @ V.double()) < 5e-5
    lik = g.likelihoods.GaussianLikelihood().to(dev)
    Ma = _gp_class(g, lambda: kern)
    m = Ma(xd, y2.float().to(dev), lik).to(dev)
    lik.noise = 0.1
    m.train()
    lik.train()
    with g.settings.max_cholesky_size(10_000):
        val = g.ExactMarginalLogLikelihood(lik, m)(m(xd), y2.float().to(dev))
    ref = OG.dense_log_prob(Kref + 0.1 * torch.eye(n2, dtype=torch.float64), y2) / n2
    assert abs(float(val) - float(ref)) < 2e-4 * max(1.0, abs(float(ref)))
