"""GPU: the product of two stationary families as ONE matrix-free operator (``KIND_PROD``; csrc/kv_directp.hpp, the product variant of
csrc/kv_grad.hpp, ``kernels.product_factors``).

Oracle: tests/product_ref.py, a float64 restatement written from the formulas.  Inputs are uniform in [0, 1]^d and lengthscales lie in 0.3 .. 0.8;
every test asserts that between 5 % and 95 % of K lies in (0.05, 0.95), so neither factor is degenerate.  Bounds:
  * K V: per column, relative to the column's largest reference entry, 2e-5 -- what tests/test_gpu_kv_split.py::_check_direct imposes on the kernel
    this one is derived from (the extra factor adds one rounding and one direct-difference generation, both near 1e-7);
  * entries of K (dense, rows, diagonal) and rows of the pivoted-Cholesky factor, max-normalised: 1e-5, the bound tests/test_gpu_compose.py puts on
    the dense form of this product;
  * gradients: 2e-3, the project's bound for every family;
  * the model: the settings and bounds of tests/test_gpu_piecewise.py (marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on
    the BBMM branch; posterior 2e-3, 5e-2 with fast_pred_var)."""
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from oracle import kernels as OK
from oracle import pivoted_cholesky as OPC
from tests.product_ref import FAMILIES, PAIRS, factor_cov, prod_cov
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

# (n, m, D_A, D_B, t); m = 0: the same cloud.  The last one exercises two row tiles per wave (NI = 2); (3, 2) completes the (D_A, D_B) grid
KV_SHAPES = [(300, 0, 1, 2, 11), (257, 513, 1, 1, 1), (65, 3000, 3, 1, 4), (130, 1000, 3, 3, 32), (1000, 129, 2, 1, 33), (700, 700, 2, 2, 65),
             (200, 600, 2, 3, 70), (16_500, 300, 1, 3, 33), (150, 260, 3, 2, 5)]


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


def _cloud(gen, n, d):
    return _f32(torch.rand(n, d, generator=gen, dtype=torch.float64))


def _ls(gen, d):
    """d lengthscales from the short end of 0.3 .. 0.8: on [0, 1]^d longer ones leave nearly all of K inside (0.05, 0.95) -- the share every test here
    bounds by 95 % -- for every family pair; with two columns even 0.4 does, so there the draw is 0.30 .. 0.32."""
    return _f32(0.3 + (0.02 if d == 2 else 0.1) * torch.rand(d, generator=gen, dtype=torch.float64))


def _mixed(K):
    """Share of K in (0.05, 0.95): both factors vary over the cloud."""
    frac = float(((K > 0.05) & (K < 0.95)).double().mean())
    assert 0.05 < frac < 0.95, frac
    return frac


def _prep(B, X, ls, shift, code, dev):
    return B.prep_points("prod", X.float().to(dev), ls.float(), shift.float().to(dev), code)


def kv_case(ka, kb, shape, seed):
    """(X1, X2 or None, ls, D_A, V, reference K) of one product case; equal families take the canonical order of dimensions."""
    n, m, da, db, t = shape
    if ka == kb and da > db:
        da, db = db, da
    gen = torch.Generator().manual_seed(seed)
    X1 = _cloud(gen, n, da + db)
    X2 = None if m == 0 else _cloud(gen, m, da + db)
    ls = _ls(gen, da + db)
    V = torch.randn(n if m == 0 else m, t, generator=gen, dtype=torch.float64).float()
    K = prod_cov(ka, kb, da, X1, X1 if X2 is None else X2, ls)
    return X1, X2, ls, da, V, K


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{FAMILIES[a]}-{FAMILIES[b]}" for a, b in PAIRS])
def test_kv_matches_restatement(pair, dev):
    from gpytorch_amd import backend as B

    ka, kb = pair
    seen = set()
    for i, shape in enumerate(KV_SHAPES):
        X1, X2, ls, da, V, K = kv_case(ka, kb, shape, 1000 * (4 * ka + kb) + i)
        _mixed(K)
        n, d, t = X1.shape[0], X1.shape[1], V.shape[1]
        seen.add((da, d - da))
        code = B.prod_code(ka, kb, da)
        shift = X1.mean(0)
        p1 = _prep(B, X1, ls, shift, code, dev)
        p2 = p1 if X2 is None else _prep(B, X2, ls, shift, code, dev)
        assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
        ref = K @ V.double()
        err = float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())
        print("kv", FAMILIES[ka], FAMILIES[kb], shape, err)
        assert err < 2e-5, (pair, shape, err)
    if ka != kb:
        assert seen == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{FAMILIES[a]}-{FAMILIES[b]}" for a, b in PAIRS])
def test_dense_rows_diag_pivoted_cholesky(pair, dev):
    from gpytorch_amd import backend as B

    ka, kb = pair
    n, m = 300, 77
    for da, db in ((1, 2), (2, 3), (3, 3), (1, 1)) + (((3, 1),) if ka != kb else ()):
        gen = torch.Generator().manual_seed(50 * (4 * ka + kb) + 4 * da + db)
        X1, X2, ls = _cloud(gen, n, da + db), _cloud(gen, m, da + db), _ls(gen, da + db)
        code = B.prod_code(ka, kb, da)
        shift = X1.mean(0)
        p1, p2 = _prep(B, X1, ls, shift, code, dev), _prep(B, X2, ls, shift, code, dev)
        scale = torch.tensor([1.7], device=dev)
        Kref = 1.7 * prod_cov(ka, kb, da, X1, X2, ls)
        _mixed(Kref / 1.7)
        e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
        rows = torch.tensor([0, n - 1, n // 2])
        e_r = rel_err(B.kernel_rows(p1, rows, p2, scale), Kref[rows])
        q1 = _prep(B, X1[:m], ls, shift, code, dev)
        e_g = rel_err(B.kernel_diag(q1, p2, scale), Kref[:m].diagonal())
        assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n))               # x1 is x2: exact unit diagonal
        # rows of the pivoted-Cholesky factor: the device's pivots replayed in the float64 oracle (float32 ties make the sequence rounding-dependent)
        rank = 10
        Kd = 1.7 * prod_cov(ka, kb, da, X1, X1, ls)
        Lt, piv, mm = B.pivoted_cholesky(p1, scale, rank, 1e-6)
        Lref, _, gaps = OPC.pivoted_cholesky(torch.full((n,), 1.7, dtype=torch.float64), lambda p: Kd[p], rank, 1e-6, forced_pivots=piv.cpu(), return_gaps=True)
        assert mm == rank == Lref.shape[1] and max(gaps) < 1e-5, gaps
        e_p = rel_err(Lt.t(), Lref)
        print("entries", FAMILIES[ka], FAMILIES[kb], (da, db), e_d, e_r, e_g, e_p)
        assert max(e_d, e_r, e_g, e_p) < 1e-5, (pair, da, db, e_d, e_r, e_g, e_p)


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{FAMILIES[a]}-{FAMILIES[b]}" for a, b in PAIRS])
def test_bilinear_derivative(pair, dev):
    """``functions.hyper_grads`` (the product variant of kv_grad_kernel) against float64 autograd of sum W o K, W = L R^T with nine random columns:
    one lengthscale per column (ARD in both factors) and one per factor (its gradient is the sum over the factor's columns); pairs containing
    Matern-1/2 also on coincident points (x2 = x1: the r = 0 guard of each factor)."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    ka, kb = pair
    cases = [(210, 333, 1, 2, False, False), (140, 90, 2, 3, True, False)]
    if 1 in pair:
        cases.append((150, 150, 2, 2, False, True))
    for n, m, da, db, single, coincide in cases:
        gen = torch.Generator().manual_seed(7 * (4 * ka + kb) + n)
        d = da + db
        X1 = _cloud(gen, n, d)
        X2 = X1 if coincide else _cloud(gen, m, d)
        if single:
            la, lb = _ls(gen, d)[:1], _ls(gen, d)[:1]
            leaves = [la.clone().requires_grad_(True), lb.clone().requires_grad_(True)]
            ls64 = torch.cat([leaves[0].expand(da), leaves[1].expand(db)])
        else:
            leaves = [_ls(gen, d).requires_grad_(True)]
            ls64 = leaves[0]
        os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
        Lm = torch.randn(n, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(m, 9, generator=gen, dtype=torch.float64).float()
        K = prod_cov(ka, kb, da, X1, X2, ls64)
        _mixed(K.detach())
        val = (Lm.double() * ((os64 * K) @ Rm.double())).sum()
        gref = torch.autograd.grad(val, leaves + [os64])
        code = B.prod_code(ka, kb, da)
        shift = X1.mean(0)
        lsd = ls64.detach().float().to(dev).reshape(1, -1)
        osd = torch.tensor([1.3], device=dev)
        p1 = _prep(B, X1, ls64.detach(), shift, code, dev)
        p2 = p1 if coincide else _prep(B, X2, ls64.detach(), shift, code, dev)
        d_ls, d_os = hyper_grads(p1, p2, lsd, osd, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
        d_ls = d_ls.double().cpu().reshape(-1)
        got_ls = torch.stack([d_ls[:da].sum(), d_ls[da:].sum()]) if single else d_ls
        want_ls = torch.cat([g.reshape(-1) for g in gref[:-1]])
        e_ls = float((got_ls - want_ls).abs().max() / want_ls.abs().max())
        e_os = abs(float(d_os) - float(gref[-1])) / abs(float(gref[-1]))
        print("grad", FAMILIES[ka], FAMILIES[kb], (n, m, da, db), "single" if single else "ard", "coincident" if coincide else "", e_ls, e_os)
        assert e_ls < 2e-3 and e_os < 2e-3, (pair, n, m, da, db, single, coincide, e_ls, e_os)
        with pytest.raises(RuntimeError, match="prod"):                               # no input gradients off the Gram-form kernel
            hyper_grads(p1, p2, lsd, osd, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)), want_x1=True)


def _time_space_kernel(g, order, dev):
    """ScaleKernel(Matern-5/2(column 0) x RBF(columns 1, 2)) with lengthscales 0.4 and (0.3, 0.6), outputscale 1.7, the members in either order."""
    kt, ks = g.kernels.MaternKernel(nu=2.5, active_dims=[0]), g.kernels.RBFKernel(active_dims=[1, 2], ard_num_dims=2)
    kern = g.kernels.ScaleKernel(kt * ks if order == 0 else ks * kt).to(dev)
    kt.lengthscale, ks.lengthscale, kern.outputscale = 0.4, torch.tensor([[0.3, 0.6]]), 1.7
    return kern, kt, ks


def _time_space_ref(x1, x2, lt, lsp, os_):
    return os_ * factor_cov("matern52", x1[:, :1], x2[:, :1], lt) * factor_cov("rbf", x1[:, 1:], x2[:, 1:], lsp)


@pytest.mark.parametrize("order", [0, 1])
def test_kernel_api_builds_a_fused_product(order, dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    gen = torch.Generator().manual_seed(11 + order)
    n, m = 500, 333
    x, x2 = _cloud(gen, n, 3), _cloud(gen, m, 3)
    kern, kt, ks = _time_space_kernel(g, order, dev)
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    plain = (kt * ks if order == 0 else ks * kt)(xd)
    assert isinstance(plain, FusedKernelLinearOperator) and plain.spec.kind == "prod" and plain.outputscale is None
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "prod" and op.shape == (n, n)
    lt, lsp, os_ = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in ([0.4], [0.3, 0.6], 1.7))
    lt32, lsp32 = _f32(lt.detach()), _f32(lsp.detach())
    Kref = _time_space_ref(x, x, lt32, lsp32, 1.7)
    _mixed(Kref / 1.7)
    assert rel_err(op.to_dense(), Kref) < 1e-5
    assert rel_err(kern(xd, x2d).to_dense(), _time_space_ref(x, x2, lt32, lsp32, 1.7)) < 1e-5
    V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    ref = Kref @ V.double()
    out = (op @ V.to(dev)).double().cpu()
    assert float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max()) < 2e-5
    # diag: the same inputs -> ones x outputscale; two different equally long inputs -> the elementwise product of the members' diagonals
    assert torch.allclose(kern(xd, diag=True).cpu(), torch.full((n,), 1.7))
    dref = _time_space_ref(x[:m], x2, lt32, lsp32, 1.7).diagonal()
    assert rel_err(kern(xd[:m], x2d, diag=True), dref) < 1e-5
    assert rel_err(op.diagonal(), torch.full((n,), 1.7)) < 1e-6
    # gradients of both raw lengthscales and the wrapping ScaleKernel's raw outputscale, through a product and through to_dense
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    val64 = (U.double() * (_time_space_ref(x, x, lt, lsp, os_) @ V.double())).sum()
    gref = torch.autograd.grad(val64, [lt, lsp, os_])
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    gref_d = torch.autograd.grad((W.double() * _time_space_ref(x, x, lt, lsp, os_)).sum(), [lt, lsp, os_])
    for how, want in (("matmul", gref), ("dense", gref_d)):
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        sig = lambda raw: torch.sigmoid(raw.detach().double().cpu())  # noqa: E731   (d softplus / d raw)
        got = [kt.raw_lengthscale.grad.double().cpu() / sig(kt.raw_lengthscale), ks.raw_lengthscale.grad.double().cpu() / sig(ks.raw_lengthscale),
               kern.raw_outputscale.grad.double().cpu() / sig(kern.raw_outputscale)]
        for a, b in zip(got, want):
            e = float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max())
            print("api grad", how, order, e)
            assert e < 2e-3, (how, order, a, b)
    # a sum of that product and an RBF kernel stays matrix-free and multiplies correctly
    rbf = g.kernels.ScaleKernel(g.kernels.RBFKernel()).to(dev)
    rbf.base_kernel.lengthscale, rbf.outputscale = 0.5, 0.6
    both = g.kernels.AdditiveKernel(kern, rbf)
    Ksum = Kref + 0.6 * factor_cov("rbf", x, x, _f32(torch.tensor([0.5])))
    with torch.no_grad():
        assert rel_err(both(xd) @ V.to(dev), Ksum @ V.double()) < 2e-5
        assert rel_err(both(xd).to_dense(), Ksum) < 1e-5


def test_product_is_matrix_free_at_size(dev):
    """n = 40 000, eleven columns: the device memory ``op @ V`` adds at its peak stays below 1/8 of the 4 n^2 bytes of a dense float32 K (the dense
    branch this product took before needs that K three times over); 64 rows are checked against the restatement."""
    import gpytorch_amd as g

    n, t = 40_000, 11
    gen = torch.Generator().manual_seed(5)
    x = _cloud(gen, n, 3)
    V = torch.randn(n, t, generator=gen, dtype=torch.float64).float()
    kern, kt, ks = _time_space_kernel(g, 0, dev)
    xd, Vd = x.float().to(dev), V.to(dev)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = kern(xd) @ Vd
        torch.cuda.synchronize()
        added = torch.cuda.max_memory_allocated() - base
    print("peak bytes added", added, "dense K", 4 * n * n)
    assert added < 4 * n * n / 8, added
    rows = torch.randint(0, n, (64,), generator=gen)
    Kr = _time_space_ref(x[rows], x, _f32(torch.tensor([0.4])), _f32(torch.tensor([0.3, 0.6])), 1.7)
    _mixed(Kr / 1.7)
    ref = Kr @ V.double()
    err = float(((out[rows.to(dev)].double().cpu() - ref).abs().max(0).values / ref.abs().max(0).values).max())
    assert err < 2e-5, err


def _gp_class(g, make_kernel):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = make_kernel()

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _model_kernel(g):
    return g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5, active_dims=[0]) * g.kernels.RBFKernel(active_dims=[1, 2]))


def _set_model(m, lik):
    m.covar_module.base_kernel.kernels[0].lengthscale = 0.3
    m.covar_module.base_kernel.kernels[1].lengthscale = 0.5
    m.covar_module.outputscale = 1.3
    lik.noise = 0.1


def test_gp_mll_cholesky_and_bbmm(dev):
    """ScaleKernel(Matern-5/2(time) x RBF(space)) + Gaussian noise, n = 1500: the marginal log likelihood and all hyper-parameter gradients on the
    Cholesky branch and on the BBMM branch (``max_cholesky_size(0)``, deterministic probes) against dense float64 autograd, with the settings and
    bounds of tests/test_gpu_piecewise.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    n = 1500
    X, y = make_data(n, 3)
    X, y = _f32(X), _f32(y)
    p = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.3, 0.5, 1.3, 0.1)]   # time / space lengthscale, outputscale, noise
    Kref = _time_space_ref(X, X, p[0].reshape(1), p[1].reshape(1), p[2])
    _mixed(Kref.detach() / 1.3)
    ref = OG.dense_log_prob(Kref + p[3] * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, p)
    M = _gp_class(g, lambda: _model_kernel(g))
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        assert isinstance(m.covar_module(m.train_inputs[0]), FusedKernelLinearOperator)
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
        ks = m.covar_module.base_kernel.kernels
        got = torch.tensor([float(ks[0].raw_lengthscale.grad.sum()), float(ks[1].raw_lengthscale.grad.sum()), float(m.covar_module.raw_outputscale.grad),
                            float(lik.noise_covar.raw_noise.grad.sum())], dtype=torch.float64)
        want = torch.tensor([float(gref[0]) * sp(0.3), float(gref[1]) * sp(0.5), float(gref[2]) * sp(1.3), float(gref[3]) * sp(0.1 - 1e-4)],
                            dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("mll", branch, e_v, e_g, got, want)
        assert e_v < tol_v, (branch, float(val), float(ref))
        assert e_g < tol_g, (branch, got, want)


def test_gp_posterior_fast_pred_var(dev):
    """Posterior mean and variance of the same model against the dense float64 posterior, exact and with ``fast_pred_var``: settings and bounds of
    tests/test_gpu_piecewise.py::test_gp_posterior_fast_pred_var."""
    import gpytorch_amd as g

    n, ns = 1500, 200
    X, y = make_data(n + ns, 3)
    X, y = _f32(X), _f32(y)
    Xt, yt, Xs = X[:n], y[:n], X[n:]
    lt, lsp = torch.tensor([0.3], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64)
    Lc = torch.linalg.cholesky(_time_space_ref(Xt, Xt, lt, lsp, 1.3) + 0.1 * torch.eye(n, dtype=torch.float64))
    Ks = _time_space_ref(Xs, Xt, lt, lsp, 1.3)
    _mixed(Ks / 1.3)
    mu_ref = (Ks @ torch.cholesky_solve(yt.unsqueeze(-1), Lc)).squeeze(-1)
    var_ref = 1.3 + 0.1 - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)
    M = _gp_class(g, lambda: _model_kernel(g))
    S = g.settings
    for fast in (True, False):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(Xt.float().to(dev), yt.float().to(dev), lik).to(dev)
        _set_model(m, lik)
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


def test_existing_dense_branches_are_untouched(dev):
    """What the rule declines keeps the dense path, value for value: a Periodic member next to a Matern, and float64 inputs."""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.operators import DenseLinearOperator

    gen = torch.Generator().manual_seed(2)
    x = _cloud(gen, 200, 2)
    kern = (g.kernels.MaternKernel(nu=1.5, active_dims=[0]) * g.kernels.PeriodicKernel(active_dims=[1])).to(dev)
    out = kern(x.float().to(dev))
    assert isinstance(out, DenseLinearOperator)
    members = kern.kernels[0](x.float().to(dev)).to_dense() * kern.kernels[1](x.float().to(dev)).to_dense()
    assert torch.equal(operators.to_dense(out), members)
    k64 = (g.kernels.RBFKernel(active_dims=[0]) * g.kernels.MaternKernel(nu=2.5, active_dims=[1])).to(dev).double()
    o64 = k64(x.to(dev))
    assert isinstance(o64, DenseLinearOperator)
    l0 = math.log(2.0)
    assert rel_err(operators.to_dense(o64), OK.rbf(x[:, :1], x[:, :1], l0, x1_eq_x2=True, direct=True) * OK.matern(x[:, 1:], x[:, 1:], l0, 2.5, x1_eq_x2=True, direct=True)) < 1e-10
