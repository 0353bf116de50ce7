"""GPU: first-order additive structure as ONE matrix-free operator (``KIND_ADD``; csrc/kv_directadd.hpp, the additive variant of csrc/kv_grad.hpp,
``kernels.AdditiveStructureKernel``).

Oracle: tests/additive_ref.py, a float64 restatement written from the formulas and pinned to the reference's own outputs
(tests/test_additive_cpu.py).  Clouds are uniform on [0, 1]^d, lengthscales are drawn from 0.2 .. 0.35 per dimension, and in every K V and
derivative case one of the two clouds is a LATTICE cloud (each coordinate one of 7 equally spaced values): at least 1 - (6/7)^2 = 26 % of its
pairs share a coordinate while differing in another, so a generated value mixes terms at rho_q = 0 with non-zero ones.  Every test asserts its
precondition (``_mixed``): in every dimension at least 5 % of the pairs have k'_q < 0.2 and at least 5 % have k'_q > 0.8.  Bounds -- those of
tests/test_gpu_product.py; the family sums same-signed terms of the same accuracy, so they carry over:
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
from tests.additive_ref import FAMILIES, add_cov, add_mean, add_terms
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

# (n, m, d, t); m = 0: the same cloud.  Every d, fewer rows than one tile, ragged ends, every column-group boundary (1, 4, 5, 32, 33, 65, 70), two row
# tiles per wave (16 500 rows)
KV_SHAPES = [(300, 0, 2, 11), (257, 513, 3, 1), (65, 3000, 4, 4), (130, 1000, 5, 32), (1000, 129, 6, 33), (700, 700, 7, 65), (200, 600, 8, 70),
             (16_500, 300, 3, 33), (150, 260, 8, 5)]
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
    return _f32(0.2 + 0.15 * torch.rand(d, generator=gen, dtype=torch.float64))


def _mixed(terms):
    """``terms`` [..., d], the one-dimensional covariances of the pairs: in every dimension >= 5 % below 0.2 and >= 5 % above 0.8."""
    t = terms.detach().reshape(-1, terms.shape[-1])
    lo, hi = (t < 0.2).double().mean(0), (t > 0.8).double().mean(0)
    assert float(lo.min()) >= 0.05 and float(hi.min()) >= 0.05, (lo, hi)


def _shares_a_coordinate(X1, X2):
    """Share of the pairs that coincide in at least one coordinate while differing in another."""
    eq = X1.unsqueeze(1) == X2.unsqueeze(0)
    return float((eq.any(-1) & ~eq.all(-1)).double().mean())


def _prep(B, X, ls, shift, kind, dev):
    return B.prep_points("add", X.float().to(dev), ls.float(), shift.float().to(dev), B.add_code(kind))


def _base(g, kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=NU[kind], **kw)


def _asq(g, base, d):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return g.kernels.AdditiveStructureKernel(base, num_dims=d)


@pytest.mark.parametrize("kind", FAMILIES)
def test_kv_matches_restatement(kind, dev):
    from gpytorch_amd import backend as B

    for i, (n, m, d, t) in enumerate(KV_SHAPES):
        gen = torch.Generator().manual_seed(1000 * FAMILIES.index(kind) + i)
        if m == 0:
            X1, X2 = _lattice(gen, n, d), None
        elif i % 2:
            X1, X2 = _lattice(gen, n, d), _cloud(gen, m, d)
        else:
            X1, X2 = _cloud(gen, n, d), _lattice(gen, m, d)
        ls = _ls(gen, d)
        V = torch.randn(n if m == 0 else m, t, generator=gen, dtype=torch.float64).float()
        terms = add_terms(kind, X1, X1 if X2 is None else X2, ls)
        _mixed(terms)
        if m == 0:
            assert _shares_a_coordinate(X1, X1) >= 0.2
        K = terms.mean(-1)
        shift = X1.mean(0)
        p1 = _prep(B, X1, ls, shift, kind, dev)
        p2 = p1 if X2 is None else _prep(B, X2, ls, shift, kind, dev)
        assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
        ref = K @ V.double()
        err = float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())
        print("kv", kind, (n, m, d, t), err)
        assert err < 2e-5, (kind, (n, m, d, t), err)


@pytest.mark.parametrize("kind", FAMILIES)
def test_dense_rows_diag_pivoted_cholesky(kind, dev):
    from gpytorch_amd import backend as B

    n, m = 300, 77
    for d in (2, 5, 8):
        gen = torch.Generator().manual_seed(50 * FAMILIES.index(kind) + d)
        X1, X2, ls = _cloud(gen, n, d), _cloud(gen, m, d), _ls(gen, d)
        shift = X1.mean(0)
        p1, p2 = _prep(B, X1, ls, shift, kind, dev), _prep(B, X2, ls, shift, kind, dev)
        assert p1.dp == (4 if d <= 4 else 8) and bool(torch.isnan(p1.xp[:, d:]).all()) and bool(torch.isfinite(p1.xp[:, :d]).all())
        scale = torch.tensor([1.7], device=dev)
        _mixed(add_terms(kind, X1, X2, ls))
        Kref = 1.7 * add_mean(kind, X1, X2, ls)
        e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
        rows = torch.tensor([0, n - 1, n // 2])
        e_r = rel_err(B.kernel_rows(p1, rows, p2, scale), Kref[rows])
        q1 = _prep(B, X1[:m], ls, shift, kind, dev)
        e_g = rel_err(B.kernel_diag(q1, p2, scale), Kref[:m].diagonal())
        assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n))               # exact unit diagonal: the library evaluates the mean
        # rows of the pivoted-Cholesky factor: the device's pivots replayed in the float64 oracle (float32 ties make the sequence rounding-dependent)
        rank = 10
        Kd = 1.7 * add_mean(kind, X1, X1, ls)
        Lt, piv, mm = B.pivoted_cholesky(p1, scale, rank, 1e-6)
        Lref, _, gaps = OPC.pivoted_cholesky(torch.full((n,), 1.7, dtype=torch.float64), lambda p: Kd[p], rank, 1e-6, forced_pivots=piv.cpu(), return_gaps=True)
        assert mm == rank == Lref.shape[1] and max(gaps) < 1e-5, gaps
        e_p = rel_err(Lt.t(), Lref)
        print("entries", kind, d, e_d, e_r, e_g, e_p)
        assert max(e_d, e_r, e_g, e_p) < 1e-5, (kind, d, e_d, e_r, e_g, e_p)


@pytest.mark.parametrize("kind", FAMILIES)
def test_bilinear_derivative(kind, dev):
    """``functions.hyper_grads`` (the additive variant of kv_grad_kernel) against float64 autograd of sum W o (s K~), W = L R^T with nine random
    columns: one lengthscale per dimension, one shared lengthscale at d = 8 (its gradient is the sum over the dimensions), and x2 = x1 on the lattice
    cloud -- every family, where a quarter of the off-diagonal pairs has a term at rho_q = 0."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    for n, m, d, single, coincide in [(210, 333, 3, False, False), (140, 90, 8, True, False), (150, 150, 4, False, True)]:
        gen = torch.Generator().manual_seed(7 * FAMILIES.index(kind) + n)
        X1 = _lattice(gen, n, d)
        X2 = X1 if coincide else _cloud(gen, m, d)
        if coincide:
            assert _shares_a_coordinate(X1, X1) >= 0.2
        leaf = (_ls(gen, d)[:1] if single else _ls(gen, d)).requires_grad_(True)
        ls64 = leaf.expand(d) if single else leaf
        os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
        Lm = torch.randn(n, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(m, 9, generator=gen, dtype=torch.float64).float()
        terms = add_terms(kind, X1, X2, ls64)
        _mixed(terms)
        val = (Lm.double() * ((os64 * terms.mean(-1)) @ Rm.double())).sum()
        g_ls, g_os = torch.autograd.grad(val, [leaf, os64])
        shift = X1.mean(0)
        lsd = ls64.detach().float().to(dev).reshape(1, -1)
        osd = torch.tensor([1.3], device=dev)
        p1 = _prep(B, X1, ls64.detach(), shift, kind, dev)
        p2 = p1 if coincide else _prep(B, X2, ls64.detach(), shift, kind, dev)
        d_ls, d_os = hyper_grads(p1, p2, lsd, osd, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)))
        d_ls = d_ls.double().cpu().reshape(-1)
        assert d_ls.numel() == d and bool(torch.isfinite(d_ls).all())
        got_ls = d_ls.sum().reshape(1) if single else d_ls
        e_ls = float((got_ls - g_ls.reshape(-1)).abs().max() / g_ls.abs().max())
        e_os = abs(float(d_os) - float(g_os)) / abs(float(g_os))
        print("grad", kind, (n, m, d), "single" if single else "ard", "coincident" if coincide else "", e_ls, e_os)
        assert e_ls < 2e-3 and e_os < 2e-3, (kind, n, m, d, single, coincide, e_ls, e_os)
        with pytest.raises(RuntimeError, match="'add'"):                              # no input gradients on the native path
            hyper_grads(p1, p2, lsd, osd, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)), want_x1=True)


def _api_kernel(g, kind, d, ls, dev, where):
    """ScaleKernel(ASK(base)) (``outer``) or ASK(ScaleKernel(base)) (``inner``), base with ARD lengthscales ``ls``, outputscale 1.7."""
    base = _base(g, kind, ard_num_dims=d)
    if where == "outer":
        kern = g.kernels.ScaleKernel(_asq(g, base, d)).to(dev)
        sk = kern
    else:
        sk = g.kernels.ScaleKernel(base)
        kern = _asq(g, sk, d).to(dev)
    base.lengthscale, sk.outputscale = ls.float().reshape(1, d), 1.7
    return kern, base, sk


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("where", ["outer", "inner"])
def test_kernel_api_builds_a_fused_additive_operator(kind, where, dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    d, n, m = 5, 500, 333
    gen = torch.Generator().manual_seed(11 + FAMILIES.index(kind))
    x, x2, ls = _lattice(gen, n, d), _cloud(gen, m, d), _ls(gen, d)
    kern, base, sk = _api_kernel(g, kind, d, ls, dev, where)
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "add" and op.shape == (n, n)
    _mixed(add_terms(kind, x, x, ls))
    Kref = 1.7 * add_cov(kind, x, x, ls)
    assert rel_err(op.to_dense(), Kref) < 1e-5
    assert rel_err(kern(xd, x2d).to_dense(), 1.7 * add_cov(kind, x, x2, ls)) < 1e-5
    V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    ref = Kref @ V.double()
    out = (op @ V.to(dev)).detach().double().cpu()
    assert float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max()) < 2e-5
    # diag: the same input -> d x outputscale, no launch; two different equally long inputs -> the elementwise sums
    assert torch.allclose(kern(xd, diag=True).cpu(), torch.full((n,), d * 1.7))
    assert rel_err(kern(xd[:m], x2d, diag=True), 1.7 * add_cov(kind, x[:m], x2, ls, diag=True)) < 1e-5
    assert rel_err(op.diagonal(), torch.full((n,), d * 1.7)) < 1e-6
    # the product equals what today's expression of the same model gives on the same device: AdditiveKernel of d one-dimensional members, tied values
    members = []
    for q in range(d):
        mk = g.kernels.ScaleKernel(_base(g, kind, active_dims=[q]))
        mk.base_kernel.lengthscale, mk.outputscale = float(ls[q]), 1.7
        members.append(mk)
    old = g.kernels.AdditiveKernel(*members).to(dev)
    with torch.no_grad():
        old_out = (old(xd) @ V.to(dev)).double().cpu()
    assert float(((out - old_out).abs().max(0).values / old_out.abs().max(0).values).max()) < 2e-5
    # gradients of the raw lengthscales and the raw outputscale, through a product and through to_dense
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    l64, o64 = ls.clone().requires_grad_(True), torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    gref = torch.autograd.grad((U.double() * ((o64 * add_cov(kind, x, x, l64)) @ V.double())).sum(), [l64, o64])
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    gref_d = torch.autograd.grad((W.double() * (o64 * add_cov(kind, x, x, l64))).sum(), [l64, o64])
    for how, want in (("matmul", gref), ("dense", gref_d)):
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        sig = lambda raw: torch.sigmoid(raw.detach().double().cpu())  # noqa: E731   (d softplus / d raw)
        got = [base.raw_lengthscale.grad.double().cpu() / sig(base.raw_lengthscale), sk.raw_outputscale.grad.double().cpu() / sig(sk.raw_outputscale)]
        for a, b in zip(got, want):
            e = float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max())
            print("api grad", kind, where, how, e)
            assert e < 2e-3, (how, a, b)
    # + with another fused kernel stays matrix-free and multiplies correctly
    rbf = g.kernels.ScaleKernel(g.kernels.RBFKernel()).to(dev)
    rbf.base_kernel.lengthscale, rbf.outputscale = 0.5, 0.6
    both = kern + rbf
    z = x / 0.5
    Ksum = Kref + 0.6 * torch.exp(-0.5 * (z.unsqueeze(1) - z.unsqueeze(0)).pow(2).sum(-1))
    with torch.no_grad():
        assert rel_err(both(xd) @ V.to(dev), Ksum @ V.double()) < 2e-5
        assert rel_err(both(xd).to_dense(), Ksum) < 1e-5


def test_additive_is_matrix_free_at_size(dev):
    """n = 40 000, eleven columns, d = 6: the device memory ``op @ V`` adds at its peak stays below 1/8 of the 4 n^2 bytes of a dense float32 K (the
    reference's d x n x m tensor is six of them); 64 rows are checked against the restatement."""
    import gpytorch_amd as g

    n, t, d = 40_000, 11, 6
    gen = torch.Generator().manual_seed(5)
    x, ls = _cloud(gen, n, d), _ls(gen, d)
    V = torch.randn(n, t, generator=gen, dtype=torch.float64).float()
    kern, _, _ = _api_kernel(g, "matern52", d, ls, dev, "outer")
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
    terms = add_terms("matern52", x[rows], x, ls)
    _mixed(terms)
    ref = (1.7 * terms.sum(-1)) @ V.double()
    err = float(((out[rows.to(dev)].double().cpu() - ref).abs().max(0).values / ref.abs().max(0).values).max())
    assert err < 2e-5, err


MODEL_D, MODEL_LS, MODEL_OS, MODEL_NOISE = 4, (0.2, 0.25, 0.3, 0.35), 1.3, 0.1


def _gp_class(g):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(_asq(g, g.kernels.MaternKernel(nu=2.5, ard_num_dims=MODEL_D), MODEL_D))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _set_model(m, lik):
    m.covar_module.base_kernel.base_kernel.lengthscale = torch.tensor([MODEL_LS])
    m.covar_module.outputscale = MODEL_OS
    lik.noise = MODEL_NOISE


def test_gp_mll_cholesky_and_bbmm(dev):
    """ScaleKernel(AdditiveStructureKernel(Matern-5/2, ARD)) + Gaussian noise, n = 1500, d = 4: the marginal log likelihood and all hyper-parameter
    gradients on the Cholesky branch and on the BBMM branch (``max_cholesky_size(0)``: mBCG + SLQ with the pivoted-Cholesky preconditioner,
    deterministic probes) against dense float64 autograd, with the settings and bounds of tests/test_gpu_product.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    n, d = 1500, MODEL_D
    X, y = make_data(n, d)
    X, y = _f32(X), _f32(y)
    ls = torch.tensor(MODEL_LS, dtype=torch.float64, requires_grad=True)
    os_, nz = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (MODEL_OS, MODEL_NOISE))
    terms = add_terms("matern52", X, X, ls)
    _mixed(terms)
    ref = OG.dense_log_prob(os_ * terms.sum(-1) + nz * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, [ls, os_, nz])
    M = _gp_class(g)
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        op = m.covar_module(m.train_inputs[0])
        assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "add"
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
    """Posterior mean and variance of the same model against the dense float64 posterior, exact and with ``fast_pred_var`` (LOVE): settings and bounds
    of tests/test_gpu_product.py::test_gp_posterior_fast_pred_var; then a fantasy model on 40 more observations against the dense posterior of the
    enlarged data set.  Its bound is 4e-3: the fantasy mean is the base model's mean cache, which the bound above holds to 2e-3, plus a
    Schur-complement correction from ONE more solve with the same float32 operator, held to the same 2e-3 (at the condition number 3.9e4 of this
    model a float32 solve has little more to give: 3.9e4 x 2^-24 = 2.3e-3) -- the two add.

    One setting differs, for the EXACT variances only: ``eval_cg_tolerance`` is 1e-6, not 1e-4.  The exact variance is the prior d s + sigma^2 = 5.3 minus
    a quadratic form k*^T K^-1 k* that the 200-column mBCG solve delivers, and with 1500 points in an additive model the posterior variance is 0.103 ..
    0.106, almost the noise alone: the bound 2e-3 of that is 2e-4 absolute, 4e-5 of the quadratic form.  A residual tolerance bounds the error of the
    form only through the condition number (3.9e4 here; ``settings.rhs_refinement`` has the argument), so it has to sit well below 4e-5; the product
    model's prior is 1.3 and leaves that solve four times the room.  The bound itself stands."""
    import gpytorch_amd as g

    n, nf, ns, d = 1500, 40, 200, MODEL_D
    X, y = make_data(n + nf + ns, d)
    X, y = _f32(X), _f32(y)
    Xt, yt, Xf, yf, Xs = X[:n], y[:n], X[n : n + nf], y[n : n + nf], X[n + nf :]
    ls = torch.tensor(MODEL_LS, dtype=torch.float64)

    def dense_posterior(Xa, ya):
        Lc = torch.linalg.cholesky(MODEL_OS * add_cov("matern52", Xa, Xa, ls) + MODEL_NOISE * torch.eye(Xa.shape[0], dtype=torch.float64))
        Ks = MODEL_OS * add_cov("matern52", Xs, Xa, ls)
        mu = (Ks @ torch.cholesky_solve(ya.unsqueeze(-1), Lc)).squeeze(-1)
        return mu, d * MODEL_OS + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)

    _mixed(add_terms("matern52", Xs, Xt, ls))
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
                S.max_root_decomposition_size(1500):
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
    """The float64 model of the same class (and a float32 one outside the rule: d = 9) is formed by ``additive_dense``: a DenseLinearOperator equal to
    the oracle to 1e-10 (float64) -- value for value what the reference's arithmetic gives."""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.operators import DenseLinearOperator

    gen = torch.Generator().manual_seed(2)
    for kind in FAMILIES:
        for d, ard in ((4, True), (9, False)):
            x, x2 = _cloud(gen, 200, d), _cloud(gen, 77, d)
            ls = _ls(gen, d) if ard else _ls(gen, d)[:1]
            base = _base(g, kind, ard_num_dims=d if ard else None)
            kern = g.kernels.ScaleKernel(_asq(g, base, d)).to(dev).double()
            base.lengthscale, kern.outputscale = ls.reshape(1, -1), 1.3
            lsv, osv = base.lengthscale.detach().double().cpu().reshape(-1), float(kern.outputscale.detach())
            for a, b in ((x, x), (x, x2)):
                out = kern(a.to(dev), b.to(dev))
                assert isinstance(out, DenseLinearOperator)
                assert rel_err(operators.to_dense(out), osv * add_cov(kind, a, b, lsv)) < 1e-10
            assert rel_err(kern(x.to(dev), diag=True), torch.full((200,), osv * d, dtype=torch.float64)) < 1e-10
            if d == 9:   # float32 beyond the native envelope: the dense branch too
                k32 = g.kernels.ScaleKernel(_asq(g, _base(g, kind), d)).to(dev)
                k32.base_kernel.base_kernel.lengthscale, k32.outputscale = float(ls[0]), 1.3
                o32 = k32(x.float().to(dev))
                assert isinstance(o32, DenseLinearOperator)
                if kind == "rbf":   # (the Matern families take the square root of the reference's float32 Gram-trick distance: no 1e-5 there)
                    assert rel_err(operators.to_dense(o32), 1.3 * add_cov(kind, x, x, _f32(k32.base_kernel.base_kernel.lengthscale.detach().cpu()).reshape(-1))) < 1e-5
