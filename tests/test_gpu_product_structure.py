"""GPU: product structure as ONE matrix-free operator (``KIND_PS``, the tensor-product Matern family; csrc/kv_directps.hpp, csrc/kv_grad_ps.hpp,
``kernels.ProductStructureKernel``), modelled on tests/test_gpu_additive.py test for test.

Oracle: tests/product_structure_ref.py, a float64 restatement written from the formulas and pinned to the reference's own outputs
(tests/test_product_structure_cpu.py).  Clouds are uniform on [0, 1]^d and in every K V and derivative case one of the two clouds is a LATTICE cloud
(each coordinate one of 7 equally spaced values), so pairs share a coordinate (r_q = 0) while differing in another.  Lengthscales are drawn from
0.5 .. 0.9 per dimension: with the additive test's 0.2 .. 0.35 the product of 8 factors is below 1e-4 for essentially every pair and a test relative
to the column maximum would see the diagonal only.  Every K V and derivative case asserts its precondition (``_mixed``): in every dimension at least
5 % of the pairs have k'_q < 0.6 and at least 5 % have k'_q > 0.9, and at least 20 % of the pairs have 0.02 < k < 0.9.  Bounds -- those of
tests/test_gpu_additive.py / tests/test_gpu_product.py; k <= 1 is a product of at most 8 factors good to a few float32 ulp each and one exponential
with an argument error <= eps sum r_q, ~1e-6 absolute together, under the f16 hi/lo split's own error, so they carry over:
  * K V: per column, relative to the column's largest reference entry, 2e-5;
  * entries of K (dense, rows, diagonal) and rows of the pivoted-Cholesky factor, max-normalised: 1e-5;
  * gradients: 2e-3;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3, 5e-2 with fast_pred_var."""
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from oracle import pivoted_cholesky as OPC
from tests.product_structure_ref import MATERN, ps_cov, ps_terms
from tests.test_gpu_additive import KV_SHAPES
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


def _cloud(gen, n, d):
    return _f32(torch.rand(n, d, generator=gen, dtype=torch.float64))


def _lattice(gen, n, d):
    """Each coordinate one of 7 equally spaced values of [0, 1]."""
    return _f32(torch.randint(0, 7, (n, d), generator=gen).double() / 6.0)


def _ls(gen, d):
    return _f32(0.5 + 0.4 * torch.rand(d, generator=gen, dtype=torch.float64))


def _mixed(terms):
    """``terms`` [..., d], the one-dimensional covariances of the pairs: in every dimension >= 5 % below 0.6 and >= 5 % above 0.9; >= 20 % of the
    pairs with 0.02 < k < 0.9."""
    t = terms.detach().reshape(-1, terms.shape[-1])
    lo, hi = (t < 0.6).double().mean(0), (t > 0.9).double().mean(0)
    k = t.prod(-1)
    mid = float(((k > 0.02) & (k < 0.9)).double().mean())
    assert float(lo.min()) >= 0.05 and float(hi.min()) >= 0.05 and mid >= 0.2, (lo, hi, mid)


def _shares_a_coordinate(X1, X2):
    """Share of the pairs that coincide in at least one coordinate while differing in another."""
    eq = X1.unsqueeze(1) == X2.unsqueeze(0)
    return float((eq.any(-1) & ~eq.all(-1)).double().mean())


def _prep(B, X, ls, shift, kind, dev):
    return B.prep_points("ps", X.float().to(dev), ls.float(), shift.float().to(dev), B.ps_code(kind))


def _psk(g, base, d):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return g.kernels.ProductStructureKernel(base, num_dims=d)


@pytest.mark.parametrize("kind", MATERN)
def test_kv_matches_restatement(kind, dev):
    from gpytorch_amd import backend as B

    for i, (n, m, d, t) in enumerate(KV_SHAPES):
        gen = torch.Generator().manual_seed(1000 * MATERN.index(kind) + i)
        if m == 0:
            X1, X2 = _lattice(gen, n, d), None
        elif i % 2:
            X1, X2 = _lattice(gen, n, d), _cloud(gen, m, d)
        else:
            X1, X2 = _cloud(gen, n, d), _lattice(gen, m, d)
        ls = _ls(gen, d)
        V = torch.randn(n if m == 0 else m, t, generator=gen, dtype=torch.float64).float()
        terms = ps_terms(kind, X1, X1 if X2 is None else X2, ls)
        _mixed(terms)
        if m == 0:
            assert _shares_a_coordinate(X1, X1) >= 0.2
        K = terms.prod(-1)
        shift = X1.mean(0)
        p1 = _prep(B, X1, ls, shift, kind, dev)
        p2 = p1 if X2 is None else _prep(B, X2, ls, shift, kind, dev)
        assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
        ref = K @ V.double()
        err = float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())
        print("kv", kind, (n, m, d, t), err)
        assert err < 2e-5, (kind, (n, m, d, t), err)


@pytest.mark.parametrize("kind", MATERN)
def test_dense_rows_diag_pivoted_cholesky(kind, dev):
    from gpytorch_amd import backend as B

    n, m = 300, 77
    for d in (2, 5, 8):
        gen = torch.Generator().manual_seed(50 * MATERN.index(kind) + d)
        X1, X2, ls = _cloud(gen, n, d), _cloud(gen, m, d), _ls(gen, d)
        shift = X1.mean(0)
        p1, p2 = _prep(B, X1, ls, shift, kind, dev), _prep(B, X2, ls, shift, kind, dev)
        assert p1.dp == (4 if d <= 4 else 8) and bool(torch.isfinite(p1.xp).all())
        assert torch.equal(p1.xp[:, d:], torch.zeros(n, p1.dp - d, device=dev))          # the base family's rows: zero padding
        scale = torch.tensor([1.7], device=dev)
        _mixed(ps_terms(kind, X1, X2, ls))
        Kref = 1.7 * ps_cov(kind, X1, X2, ls)
        e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
        rows = torch.tensor([0, n - 1, n // 2])
        e_r = rel_err(B.kernel_rows(p1, rows, p2, scale), Kref[rows])
        q1 = _prep(B, X1[:m], ls, shift, kind, dev)
        e_g = rel_err(B.kernel_diag(q1, p2, scale), Kref[:m].diagonal())
        assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n))                    # exact unit diagonal
        # rows of the pivoted-Cholesky factor: the device's pivots replayed in the float64 oracle (float32 ties make the sequence rounding-dependent)
        rank = 10
        Kd = 1.7 * ps_cov(kind, X1, X1, ls)
        Lt, piv, mm = B.pivoted_cholesky(p1, scale, rank, 1e-6)
        assert piv is None                                                                # (the row-built factor: its pivots are read off its rows)
        piv = _pivots_of(Lt, 1.7)
        Lref, _, gaps = OPC.pivoted_cholesky(torch.full((n,), 1.7, dtype=torch.float64), lambda p: Kd[p], rank, 1e-6, forced_pivots=piv.cpu(), return_gaps=True)
        assert mm == rank == Lref.shape[1] and max(gaps) < 1e-5, gaps
        e_p = rel_err(Lt.t(), Lref)
        print("entries", kind, d, e_d, e_r, e_g, e_p)
        assert max(e_d, e_r, e_g, e_p) < 1e-5, (kind, d, e_d, e_r, e_g, e_p)


def _pivots_of(Lt, kdiag):
    """The pivot sequence of a row-built pivoted-Cholesky factor Lt [rank, n] (``bbmm.pivoted_cholesky_rows`` returns no pivots): step k sets
    L[k, p_k] = sqrt(residual diagonal at p_k), so after it the residual diagonal kdiag - sum_{j<=k} L[j]^2 vanishes at p_k (to float32 rounding) and
    stays positive at every point not chosen yet."""
    L = Lt.double().cpu()
    resid, used, piv = torch.full((L.shape[1],), float(kdiag), dtype=torch.float64), torch.zeros(L.shape[1], dtype=torch.bool), []
    for k in range(L.shape[0]):
        resid = resid - L[k] ** 2
        p = int(torch.where(used, torch.full_like(resid, float("inf")), resid).argmin())
        assert abs(float(resid[p])) < 1e-5 * float(kdiag) and float(L[k, p]) > 0
        piv.append(p)
        used[p] = True
    return torch.tensor(piv)


@pytest.mark.parametrize("kind", MATERN)
def test_bilinear_derivative(kind, dev):
    """``functions.hyper_grads`` (csrc/kv_grad_ps.hpp) against float64 autograd of sum W o (s K), W = L R^T with nine random columns: one
    lengthscale per dimension at d = 3, one shared lengthscale at d = 8 (its gradient is the sum over the dimensions), and x2 = x1 on the lattice
    cloud, where a quarter of the off-diagonal pairs has r_q = 0 in some q.  Two calls give identical bits; input gradients are refused."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    for n, m, d, single, coincide in [(210, 333, 3, False, False), (140, 90, 8, True, False), (150, 150, 4, False, True)]:
        gen = torch.Generator().manual_seed(7 * MATERN.index(kind) + n)
        X1 = _lattice(gen, n, d)
        X2 = X1 if coincide else _cloud(gen, m, d)
        if coincide:
            assert _shares_a_coordinate(X1, X1) >= 0.2
        leaf = (_ls(gen, d)[:1] if single else _ls(gen, d)).requires_grad_(True)
        ls64 = leaf.expand(d) if single else leaf
        os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
        Lm = torch.randn(n, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(m, 9, generator=gen, dtype=torch.float64).float()
        terms = ps_terms(kind, X1, X2, ls64)
        _mixed(terms)
        val = (Lm.double() * ((os64 * terms.prod(-1)) @ Rm.double())).sum()
        g_ls, g_os = torch.autograd.grad(val, [leaf, os64])
        shift = X1.mean(0)
        lsd = ls64.detach().float().to(dev).reshape(1, -1)
        osd = torch.tensor([1.3], device=dev)
        p1 = _prep(B, X1, ls64.detach(), shift, kind, dev)
        p2 = p1 if coincide else _prep(B, X2, ls64.detach(), shift, kind, dev)
        lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
        d_ls, d_os = hyper_grads(p1, p2, lsd, osd, lt, rt)
        s1, s2 = B.kv_grad_ps(p1, p2, lt, rt), B.kv_grad_ps(p1, p2, lt, rt)
        assert s1.shape == (1 + d,) and torch.equal(s1, s2)                           # fixed-order float64 accumulation, no atomics
        d_ls = d_ls.double().cpu().reshape(-1)
        assert d_ls.numel() == d and bool(torch.isfinite(d_ls).all())
        got_ls = d_ls.sum().reshape(1) if single else d_ls
        e_ls = float((got_ls - g_ls.reshape(-1)).abs().max() / g_ls.abs().max())
        e_os = abs(float(d_os) - float(g_os)) / abs(float(g_os))
        print("grad", kind, (n, m, d), "single" if single else "ard", "coincident" if coincide else "", e_ls, e_os)
        assert e_ls < 2e-3 and e_os < 2e-3, (kind, n, m, d, single, coincide, e_ls, e_os)
        with pytest.raises(RuntimeError, match="'ps'"):                               # no input gradients on the native path
            hyper_grads(p1, p2, lsd, osd, lt, rt, want_x1=True)


def _api_kernel(g, kind, d, ls, dev, where):
    """ScaleKernel(PSK(base)) (``outer``) or PSK(ScaleKernel(base)) (``inner``), base with ARD lengthscales ``ls``, outputscale 1.2."""
    base = g.kernels.MaternKernel(nu=NU[kind], ard_num_dims=d)
    if where == "outer":
        kern = g.kernels.ScaleKernel(_psk(g, base, d)).to(dev)
        sk = kern
    else:
        sk = g.kernels.ScaleKernel(base)
        kern = _psk(g, sk, d).to(dev)
    base.lengthscale, sk.outputscale = ls.float().reshape(1, d), 1.2
    return kern, base, sk


@pytest.mark.parametrize("kind", ["matern12", "matern52"])
@pytest.mark.parametrize("where", ["outer", "inner"])
def test_kernel_api_builds_a_fused_product_structure_operator(kind, where, dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    d, n, m = 5, 500, 333
    gen = torch.Generator().manual_seed(11 + MATERN.index(kind))
    x, x2, ls = _lattice(gen, n, d), _cloud(gen, m, d), _ls(gen, d)
    kern, base, sk = _api_kernel(g, kind, d, ls, dev, where)
    pw = 1 if where == "outer" else d                                                 # an inner outputscale enters as s^d
    S = 1.2 ** pw
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "ps" and op.shape == (n, n)
    _mixed(ps_terms(kind, x, x, ls))
    Kref = S * ps_cov(kind, x, x, ls)
    assert rel_err(op.to_dense(), Kref) < 1e-5
    assert rel_err(kern(xd, x2d).to_dense(), S * ps_cov(kind, x, x2, ls)) < 1e-5
    V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    ref = Kref @ V.double()
    out = (op @ V.to(dev)).detach().double().cpu()
    assert float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max()) < 2e-5
    # diag: the same input -> s^d, no launch; two different equally long inputs -> the elementwise products
    assert torch.allclose(kern(xd, diag=True).cpu(), torch.full((n,), S))
    assert rel_err(kern(xd[:m], x2d, diag=True), S * ps_cov(kind, x[:m], x2, ls, diag=True)) < 1e-5
    assert rel_err(op.diagonal(), torch.full((n,), S)) < 1e-6
    # gradients of the raw lengthscales and the raw outputscale (inside: d s^(d-1)), through a product and through to_dense
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    l64, o64 = ls.clone().requires_grad_(True), torch.tensor(1.2, dtype=torch.float64, requires_grad=True)
    gref = torch.autograd.grad((U.double() * ((o64 ** pw * ps_cov(kind, x, x, l64)) @ V.double())).sum(), [l64, o64])
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    gref_d = torch.autograd.grad((W.double() * (o64 ** pw * ps_cov(kind, x, x, l64))).sum(), [l64, o64])
    for how, want in (("matmul", gref), ("dense", gref_d)):
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        sig = lambda raw: torch.sigmoid(raw.detach().double().cpu())  # noqa: E731   (d softplus / d raw)
        assert base.raw_lengthscale.grad is not None and sk.raw_outputscale.grad is not None
        got = [base.raw_lengthscale.grad.double().cpu() / sig(base.raw_lengthscale), sk.raw_outputscale.grad.double().cpu() / sig(sk.raw_outputscale)]
        for a, b in zip(got, want):
            e = float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max())
            print("api grad", kind, where, how, e)
            assert e < 2e-3, (how, a, b)


def test_product_structure_is_matrix_free_at_size(dev):
    """n = 60 000, eleven columns, d = 6: ``op @ V`` completes and the device memory it adds at its peak (measured as tests/test_gpu_additive.py
    measures it) is far below the d n^2 4 bytes of the reference's d x n x n tensor (86 GB) -- below 1 GB --; 64 rows are checked against the restatement."""
    import gpytorch_amd as g

    n, t, d = 60_000, 11, 6
    gen = torch.Generator().manual_seed(5)
    x, ls = _cloud(gen, n, d), _ls(gen, d)
    V = torch.randn(n, t, generator=gen, dtype=torch.float64).float()
    kern, _, _ = _api_kernel(g, "matern52", d, ls, dev, "outer")
    xd, Vd = x.float().to(dev), V.to(dev)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()                      # (what earlier tests of the process still hold is not this product's)
        out = kern(xd) @ Vd
        torch.cuda.synchronize()
        added = torch.cuda.max_memory_allocated() - base
    print("peak bytes added", added, "d x n x n float32", 4 * d * n * n)
    assert added < 1e9, added
    rows = torch.randint(0, n, (64,), generator=gen)
    terms = ps_terms("matern52", x[rows], x, ls)
    _mixed(terms)
    ref = (1.2 * terms.prod(-1)) @ V.double()
    err = float(((out[rows.to(dev)].double().cpu() - ref).abs().max(0).values / ref.abs().max(0).values).max())
    print("kv at size", err)
    assert err < 2e-5, err


MODEL_D, MODEL_LS, MODEL_OS, MODEL_NOISE = 4, (0.5, 0.6, 0.7, 0.8), 1.3, 0.1


def _gp_class(g):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(_psk(g, g.kernels.MaternKernel(nu=2.5, ard_num_dims=MODEL_D), MODEL_D))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _set_model(m, lik):
    m.covar_module.base_kernel.base_kernel.lengthscale = torch.tensor([MODEL_LS])
    m.covar_module.outputscale = MODEL_OS
    lik.noise = MODEL_NOISE


def test_gp_mll_cholesky_and_bbmm(dev):
    """ScaleKernel(ProductStructureKernel(Matern-5/2, ARD)) + Gaussian noise, n = 600, d = 4: the marginal log likelihood and all hyper-parameter
    gradients on the Cholesky branch and on the BBMM branch (``max_cholesky_size(0)``: mBCG + SLQ with the pivoted-Cholesky preconditioner,
    deterministic probes) against dense float64 autograd, with the settings and bounds of tests/test_gpu_additive.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    n, d = 600, MODEL_D
    X, y = make_data(n, d)
    X, y = _f32(X), _f32(y)
    ls = torch.tensor(MODEL_LS, dtype=torch.float64, requires_grad=True)
    os_, nz = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (MODEL_OS, MODEL_NOISE))
    terms = ps_terms("matern52", X, X, ls)
    _mixed(terms)
    ref = OG.dense_log_prob(os_ * terms.prod(-1) + nz * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, [ls, os_, nz])
    M = _gp_class(g)
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        op = m.covar_module(m.train_inputs[0])
        assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "ps"
        mll = g.ExactMarginalLogLikelihood(lik, m)
        m.train()
        lik.train()
        S = g.settings
        with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(300), \
                S.max_preconditioner_size(15), S.deterministic_probes(True), S.max_lanczos_quadrature_iterations(100):
            warnings.simplefilter("ignore")
            torch.manual_seed(0)
            val = mll(m(m.train_inputs[0]), m.train_targets)
            val.backward()
            S.deterministic_probes.reset()
        tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
        sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731
        base = m.covar_module.base_kernel.base_kernel
        got = torch.tensor([float(v) for v in base.raw_lengthscale.grad.reshape(-1)] + [float(m.covar_module.raw_outputscale.grad),
                           float(lik.noise_covar.raw_noise.grad.sum())], dtype=torch.float64)
        want = torch.tensor([float(gref[0][q]) * sp(MODEL_LS[q]) for q in range(d)] + [float(gref[1]) * sp(MODEL_OS), float(gref[2]) * sp(MODEL_NOISE - 1e-4)],
                            dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("mll", branch, e_v, e_g, got, want)
        assert e_v < tol_v, (branch, float(val), float(ref))
        assert e_g < tol_g, (branch, got, want)


def test_gp_posterior_fast_pred_var_and_fantasy(dev):
    """Posterior mean and variance of the same model (n = 500) against the dense float64 posterior, exact and with ``fast_pred_var`` (LOVE): 2e-3, and
    5e-2 for the LOVE variances; then a fantasy model on 40 more observations against the dense posterior of the enlarged data set, at the 4e-3 that
    tests/test_gpu_additive.py derives for it (the base model's mean cache at 2e-3 plus one more float32 solve at 2e-3)."""
    import gpytorch_amd as g

    n, nf, ns, d = 500, 40, 100, MODEL_D
    X, y = make_data(n + nf + ns, d)
    X, y = _f32(X), _f32(y)
    Xt, yt, Xf, yf, Xs = X[:n], y[:n], X[n : n + nf], y[n : n + nf], X[n + nf :]
    ls = torch.tensor(MODEL_LS, dtype=torch.float64)

    def dense_posterior(Xa, ya):
        Lc = torch.linalg.cholesky(MODEL_OS * ps_cov("matern52", Xa, Xa, ls) + MODEL_NOISE * torch.eye(Xa.shape[0], dtype=torch.float64))
        Ks = MODEL_OS * ps_cov("matern52", Xs, Xa, ls)
        mu = (Ks @ torch.cholesky_solve(ya.unsqueeze(-1), Lc)).squeeze(-1)
        return mu, MODEL_OS + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)

    mu_ref, var_ref = dense_posterior(Xt, yt)
    M = _gp_class(g)
    S = g.settings
    for fast in (True, False):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(Xt.float().to(dev), yt.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        m.eval()
        lik.eval()
        torch.manual_seed(1)
        with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4 if fast else 1e-6), \
                S.max_root_decomposition_size(500):
            warnings.simplefilter("ignore")
            pred = lik(m(Xs.float().to(dev)))
            mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
        e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
        print("posterior fast_pred_var", fast, e_mu, e_var)
        assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.eval_cg_tolerance(1e-5), S.skip_posterior_variances():
        warnings.simplefilter("ignore")
        m(Xs.float().to(dev))
        fant = m.get_fantasy_model(Xf.float().to(dev), yf.float().to(dev))
        mu_f = fant(Xs.float().to(dev)).mean
    mu_full, _ = dense_posterior(torch.cat([Xt, Xf]), torch.cat([yt, yf]))
    e_f = rel_err(mu_f, mu_full)
    print("fantasy", e_f)
    assert fant.train_inputs[0].shape[0] == n + nf and e_f < 4e-3, e_f


def test_float64_model_takes_the_dense_branch(dev):
    """The float64 model of the same class (and a float32 one outside the rule: d = 9) is formed by ``ps_dense``: a DenseLinearOperator equal to the
    oracle to 1e-10 (float64)."""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.operators import DenseLinearOperator

    gen = torch.Generator().manual_seed(2)
    for kind in MATERN:
        for d, ard in ((4, True), (9, False)):
            x, x2 = _cloud(gen, 200, d), _cloud(gen, 77, d)
            ls = _ls(gen, d) if ard else _ls(gen, d)[:1]
            base = g.kernels.MaternKernel(nu=NU[kind], ard_num_dims=d if ard else None)
            kern = g.kernels.ScaleKernel(_psk(g, base, d)).to(dev).double()
            base.lengthscale, kern.outputscale = ls.reshape(1, -1), 1.3
            lsv, osv = base.lengthscale.detach().double().cpu().reshape(-1), float(kern.outputscale.detach())
            for a, b in ((x, x), (x, x2)):
                out = kern(a.to(dev), b.to(dev))
                assert isinstance(out, DenseLinearOperator)
                assert rel_err(operators.to_dense(out), osv * ps_cov(kind, a, b, lsv)) < 1e-10
            assert rel_err(kern(x.to(dev), diag=True), torch.full((200,), osv, dtype=torch.float64)) < 1e-10
            if d == 9:   # float32 beyond the native envelope: the dense branch too
                k32 = g.kernels.ScaleKernel(_psk(g, g.kernels.MaternKernel(nu=NU[kind]), d)).to(dev)
                assert isinstance(k32(x.float().to(dev)), DenseLinearOperator)


def test_rbf_base_is_the_ard_rbf_operator(dev):
    """ProductStructureKernel(RBFKernel): K V equals ``RBFKernel(ard_num_dims=d)``'s bit for bit -- the same operator (native family "rbf")."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    gen = torch.Generator().manual_seed(8)
    for d, single in ((3, False), (6, True)):
        x, x2, ls = _cloud(gen, 700, d), _cloud(gen, 300, d), _ls(gen, d)
        V = torch.randn(300, 11, generator=gen).to(dev)
        rb = g.kernels.RBFKernel(ard_num_dims=None if single else d)
        rb.lengthscale = float(ls[0]) if single else ls.float().reshape(1, d)
        kern = _psk(g, rb, d).to(dev)
        ard = g.kernels.RBFKernel(ard_num_dims=d).to(dev)
        ard.lengthscale = rb.lengthscale.detach().expand(1, d)
        xd, x2d = x.float().to(dev), x2.float().to(dev)
        with torch.no_grad():
            op = kern(xd, x2d)
            assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "rbf" and tuple(op.lengthscale.shape) == (1, d)
            assert torch.equal(op @ V, ard(xd, x2d) @ V)
            assert rel_err(op.to_dense(), ps_cov("rbf", x, x2, ls[:1].expand(d) if single else ls)) < 1e-5


GRID_M = 20


def _grid_kernel(g, dev, d, dtype=torch.float32):
    K = g.kernels
    gk = K.GridInterpolationKernel(K.RBFKernel(ard_num_dims=d), grid_size=GRID_M, num_dims=1, grid_bounds=[(0.0, 1.0)])
    kern = _psk(g, K.ScaleKernel(gk), d).to(device=dev, dtype=dtype)
    gk.base_kernel.lengthscale = torch.tensor([[0.3 + 0.15 * q for q in range(d)]])
    kern.base_kernel.outputscale = 1.1
    return kern, gk


@pytest.mark.parametrize("d", [2, 3])
def test_grid_base_is_one_exact_interpolation_operator(d, dev):
    """ProductStructureKernel over GridInterpolationKernel(num_dims=1), m = 20: ONE ``SKIFusedLinearOperator`` on d copies of the axis; K V against
    the float64 product of the d one-dimensional interpolated covariances (``dimension_batch`` in float64 on the CPU, times s^d) at the bound of
    tests/test_gpu_ski_additive.py's K V comparison (1e-5 of the largest entry); one marginal log likelihood and its gradient through it on the
    Cholesky branch (2e-4 / 3e-3) against float64 autograd through the same dense product."""
    import gpytorch_amd as g
    from gpytorch_amd.ski import SKIFusedLinearOperator

    gen = torch.Generator().manual_seed(30 + d)
    n, m = 300, 170
    x1, x2 = (0.06 + 0.88 * torch.rand(n, d, generator=gen)).float(), (0.06 + 0.88 * torch.rand(m, d, generator=gen)).float()
    kern, gk = _grid_kernel(g, dev, d)
    k64, gk64 = _grid_kernel(g, "cpu", d, torch.float64)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        op = kern(x1.to(dev), x2.to(dev))
        assert isinstance(op, SKIFusedLinearOperator) and len(op.grid) == d and len(op.columns) == d and not op.spec.additive
        sd = float(k64.base_kernel.outputscale) ** d
        want = sd * gk64.dimension_batch(x1.double(), x2.double()).prod(-3)
        got = (op @ torch.eye(m, device=dev)).double().cpu()
        e_kv = float((got - want).abs().max() / want.abs().max())
        V = torch.randn(m, 11, generator=gen)
        e_v = rel_err(op @ V.to(dev), want @ V.double())
        print("grid kv", d, e_kv, e_v)
        assert e_kv <= 1e-5 and e_v <= 1e-5
        sq = kern(x1.to(dev))
        assert isinstance(sq, SKIFusedLinearOperator) and rel_err(sq.diagonal(), (sd * gk64.dimension_batch(x1.double(), x1.double()).prod(-3)).diagonal()) <= 1e-5

    # one marginal log likelihood and its gradient
    y = (torch.sin(3.0 * x1).sum(-1) + 0.2 * torch.randn(n, generator=gen)).float()

    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik, covar):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = covar

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    model = M(x1.to(dev), y.to(dev), lik, kern).to(dev)
    lik.noise = 0.1
    model.train()
    lik.train()
    S = g.settings
    with warnings.catch_warnings(), S.max_cholesky_size(10_000), S.cg_tolerance(1e-5):
        warnings.simplefilter("ignore")
        val = g.ExactMarginalLogLikelihood(lik, model)(model(model.train_inputs[0]), model.train_targets)
        val.backward()
    raw64 = [gk64.base_kernel.raw_lengthscale, k64.base_kernel.raw_outputscale]
    nz = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    K64 = k64.base_kernel.outputscale ** d * gk64.dimension_batch(x1.double(), x1.double()).prod(-3)
    ref = OG.dense_log_prob(K64 + nz * torch.eye(n, dtype=torch.float64), y.double()) / n
    gref = torch.autograd.grad(ref, raw64 + [nz])
    want = torch.cat([gref[0].reshape(-1), gref[1].reshape(-1), gref[2].reshape(-1) * (1.0 - math.exp(-(0.1 - 1e-4)))])
    got = torch.cat([gk.base_kernel.raw_lengthscale.grad.reshape(-1), kern.base_kernel.raw_outputscale.grad.reshape(-1),
                     lik.noise_covar.raw_noise.grad.reshape(-1)]).double().cpu()
    e_val, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
    print("grid mll", d, e_val, e_g, got, want)
    assert e_val < 2e-4 and e_g < 3e-3, (float(val), float(ref), got, want)
