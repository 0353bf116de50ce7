"""GPU: the Newton-Girard additive family as ONE matrix-free operator (``GPAMD_NG``; csrc/kv_directng.hpp, csrc/kv_grad_ng.hpp,
``kernels.NewtonGirardAdditiveKernel``).

Oracle: tests/newton_girard_ref.py, float64 closed forms (elementary symmetric polynomials by enumeration of the subsets -- no recursion).  Clouds are
uniform on [0, 1]^d or LATTICE clouds (each coordinate one of 7 equally spaced values: a quarter of the pairs share a coordinate, z_q = 1 exactly, while
differing in another); FAR clouds are lattice clouds with half of the coordinates moved by an offset at which the one-dimensional covariance of the
family falls below the float32 normal range (2^-126) for every lengthscale in use -- no larger, because prepared coordinates are float32 and the offset
costs them resolution.
Bounds -- those of tests/test_gpu_additive.py, the same kernel body and split contraction:
  * K V: per column, relative to the column's largest reference entry, 2e-5;
  * entries of K (dense, rows, diagonal) and rows of the pivoted-Cholesky factor, max-normalised: 1e-5;
  * derivative sums and gradients: 2e-3;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3, 5e-2 with fast_pred_var."""
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from tests.newton_girard_ref import FAMILIES, add_terms, ng_cov, ng_cov_normalised, ng_grad_sums, ng_norm
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}
# (n, m, d, t, R, cloud); m = 0: the same cloud.  Every d at (70, 45) with R over {1, 2, 3, 4, d} (both degree caps and the zero-weight gap: R = 1, 2 at
# cap 3; R = 4 at cap d for d > 4) and t over the column-group boundaries 1, 4, 5, 32, 33, 65; fewer rows than one tile; ragged ends; two row tiles per
# wave (16 500 rows: a slice of the rows is checked) at the cap-3 and at the widest cap-8 kernel; lattice and far clouds
KV_SHAPES = [(70, 45, 2, 1, 1, "uniform"), (70, 45, 3, 4, 2, "lattice"), (70, 45, 4, 5, 3, "uniform"), (70, 45, 5, 32, 4, "lattice"),
             (70, 45, 6, 33, 6, "uniform"), (70, 45, 7, 65, 7, "lattice"), (70, 45, 8, 11, 8, "uniform"), (70, 45, 8, 5, 4, "far"),
             (70, 0, 5, 4, 2, "lattice"), (20, 300, 4, 33, 4, "far"), (333, 257, 6, 65, 3, "lattice"), (333, 0, 3, 5, 3, "far"),
             (16_500, 130, 8, 5, 8, "uniform"), (16_500, 130, 5, 33, 3, "lattice")]


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


# offset / 0.35 (the largest lengthscale drawn) beyond the point where k' < 2^-126: RBF exp(-rho^2 / 2) at rho > 13.3; Matern e^-u p(u) at u > 87.4, 92, 97
FAR_OFFSET = {"rbf": 5.0, "matern12": 31.0, "matern32": 19.0, "matern52": 16.0}


def _cloud(gen, n, d, how="uniform", kind=None):
    if how == "uniform":
        return _f32(torch.rand(n, d, generator=gen, dtype=torch.float64))
    x = torch.randint(0, 7, (n, d), generator=gen).double() / 6.0           # lattice: each coordinate one of 7 equally spaced values of [0, 1]
    if how == "far":
        x = x + FAR_OFFSET[kind] * (torch.rand(n, d, generator=gen) < 0.5)
    return _f32(x)


def _ls(gen, d):
    return _f32(0.2 + 0.15 * torch.rand(d, generator=gen, dtype=torch.float64))


def _sigma(gen, r):
    return _f32(0.2 + torch.rand(r, generator=gen, dtype=torch.float64))


def _prep(B, X, ls, shift, kind, sigma, dev):
    return B.prep_points("ng", X.float().to(dev), ls.float(), shift.float().to(dev), (B.add_code(kind), sigma.float().to(dev)))


def _base(g, kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=NU[kind], **kw)


def _ng(g, base, d, r):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return g.kernels.NewtonGirardAdditiveKernel(base, num_dims=d, max_degree=r)


def _col_err(out, ref):
    return float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())


def _check_cloud(how, terms):
    """The precondition a cloud is there for: shared coordinates (z_q = 1 exactly) next to differing ones; terms that are zero in float32."""
    t = terms.reshape(-1, terms.shape[-1])
    if how in ("lattice", "far"):
        one = t == 1.0
        assert float((one.any(-1) & ~one.all(-1)).double().mean()) >= 0.15
    if how == "far":
        assert float((t < 2.0 ** -126).any(-1).double().mean()) >= 0.3


@pytest.mark.parametrize("kind", FAMILIES)
def test_kv_matches_closed_form(kind, dev):
    from gpytorch_amd import backend as B

    for i, (n, m, d, t, r, how) in enumerate(KV_SHAPES):
        gen = torch.Generator().manual_seed(2000 * FAMILIES.index(kind) + i)
        X1 = _cloud(gen, n, d, how, kind)
        X2 = X1 if m == 0 else _cloud(gen, m, d, how, kind)
        ls, sigma = _ls(gen, d), _sigma(gen, r)
        V = torch.randn(X2.shape[0], t, generator=gen, dtype=torch.float64).float()
        rows = torch.arange(n) if n <= 1000 else torch.cat([torch.arange(0, 160), torch.arange(n - 100, n)])   # (both row tiles of a wave, the ragged end)
        _check_cloud(how, add_terms(kind, X1[rows[:200]], X2, ls))
        shift = X1.mean(0)
        p1 = _prep(B, X1, ls, shift, kind, sigma, dev)
        p2 = p1 if m == 0 else _prep(B, X2, ls, shift, kind, sigma, dev)
        assert p1.kind == "ng" and p1.param.r == r and p1.param.rc == B.ng_cap(d, r) and B.kv_flags(p1, p2, t) == B.KV_SPLIT
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
        assert bool(torch.isfinite(out).all())
        ref = ng_cov_normalised(kind, X1[rows], X2, ls, sigma) @ V.double()
        err = _col_err(out[rows], ref)
        print("kv", kind, (n, m, d, t, r, how), err)
        assert err < 2e-5, (kind, (n, m, d, t, r, how), err)
        if r == 1:   # e_1 is the additive kernel: the GPAMD_ADD product of the same inputs (its mean of d terms IS k~ at R = 1)
            q1 = B.prep_points("add", X1.float().to(dev), ls.float(), shift.float().to(dev), B.add_code(kind))
            q2 = q1 if m == 0 else B.prep_points("add", X2.float().to(dev), ls.float(), shift.float().to(dev), B.add_code(kind))
            add = B.from_probe_major(B.kv(q1, q2, B.to_probe_major(V.to(dev))), n).double().cpu()
            assert _col_err(out, add) < 2e-5


@pytest.mark.parametrize("kind", FAMILIES)
def test_bilinear_derivative_sums(kind, dev):
    """All 1 + d + rc sums of ``gpamd_kv_ng_grad_f32`` against the dense float64 sums, W = L R^T with nine random columns; the last case (one far
    cloud against itself) is the one a leave-one-out polynomial formed as a quotient by z_q would fail: a third of its z_q are exactly zero.  Error of
    a sum: relative to the largest reference sum of its group (k~ | the d per-dimension sums | the e_n sums divided by C(d, n)), 2e-3."""
    from gpytorch_amd import backend as B

    for n, m, d, r, how, coincide in [(210, 333, 3, 3, "lattice", False), (140, 90, 8, 2, "lattice", False), (150, 150, 4, 4, "lattice", True),
                                      (160, 160, 5, 5, "far", True)]:
        gen = torch.Generator().manual_seed(9 * FAMILIES.index(kind) + n)
        X1 = _cloud(gen, n, d, how, kind)
        X2 = X1 if coincide else _cloud(gen, m, d, how, kind)
        ls, sigma = _ls(gen, d), _sigma(gen, r)
        _check_cloud(how, add_terms(kind, X1, X2, ls))
        Lm = torch.randn(n, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(m, 9, generator=gen, dtype=torch.float64).float()
        rc = B.ng_cap(d, r)
        ref = ng_grad_sums(kind, X1, X2, ls, sigma, Lm.double() @ Rm.double().t(), rc)
        shift = X1.mean(0)
        p1 = _prep(B, X1, ls, shift, kind, sigma, dev)
        p2 = p1 if coincide else _prep(B, X2, ls, shift, kind, sigma, dev)
        got = B.kv_grad_ng(p1, p2, B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))).double().cpu()
        assert got.shape == ref.shape == (1 + d + rc,) and bool(torch.isfinite(got).all())
        # the prepared coordinates carry the family constant: s_q differs from the oracle's by a constant factor, (dk'/ds) s does not
        binom = torch.tensor([math.comb(d, k) for k in range(1, rc + 1)], dtype=torch.float64)
        e_k = abs(float(got[0] - ref[0])) / abs(float(ref[0]))
        e_q = float((got[1 : 1 + d] - ref[1 : 1 + d]).abs().max() / ref[1 : 1 + d].abs().max())
        e_e = float((((got[1 + d :] - ref[1 + d :]) / binom).abs().max()) / (ref[1 + d :] / binom).abs().max())
        print("grad sums", kind, (n, m, d, r, how), e_k, e_q, e_e)
        assert max(e_k, e_q, e_e) < 2e-3, (kind, (n, m, d, r, how), e_k, e_q, e_e)


@pytest.mark.parametrize("kind", FAMILIES)
def test_dense_rows_diag_pivoted_cholesky(kind, dev):
    from gpytorch_amd import backend as B

    n, m = 300, 77
    for d, r in ((2, 2), (5, 3), (8, 5)):
        gen = torch.Generator().manual_seed(60 * FAMILIES.index(kind) + d)
        X1, X2, ls, sigma = _cloud(gen, n, d), _cloud(gen, m, d), _ls(gen, d), _sigma(gen, r)
        shift = X1.mean(0)
        p1, p2 = _prep(B, X1, ls, shift, kind, sigma, dev), _prep(B, X2, ls, shift, kind, sigma, dev)
        assert p1.dp == (4 if d <= 4 else 8) and bool((p1.xp[:, d:] == 0).all())          # the base family's rows: zero padding
        S = float(ng_norm(sigma, d))
        scale = torch.tensor([S], device=dev)
        Kref = ng_cov(kind, X1, X2, ls, sigma)
        e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
        rows = torch.tensor([0, n - 1, n // 2])
        e_r = rel_err(B.kernel_rows(p1, rows, p2, scale), Kref[rows])
        q1 = _prep(B, X1[:m], ls, shift, kind, sigma, dev)
        e_g = rel_err(B.kernel_diag(q1, p2, scale), Kref[:m].diagonal())
        assert float((B.kernel_diag(p1, p1).cpu() - 1.0).abs().max()) < 1e-6               # unit diagonal: the library evaluates k / S
        # pivoted Cholesky through the row callback (no pivot sequence comes back): a greedy rank-10 factor reproduces K on its ten pivot rows and leaves a
        # non-negative diagonal -- the check of tests/test_gpu_sm.py for the other row-built family
        rank = 10
        Kd = ng_cov(kind, X1, X1, ls, sigma)
        Lt, piv, mm = B.pivoted_cholesky(p1, scale, rank, 1e-6)
        L = Lt.double().cpu().t()
        resid = Kd - L @ L.t()
        print("entries", kind, d, r, e_d, e_r, e_g, float(resid.abs().max(1).values.sort().values[rank - 1]) / S)
        assert piv is None and mm == rank and L.shape == (n, rank)
        assert int((resid.abs().max(1).values < 1e-5 * S).sum()) == rank
        assert float(resid.diagonal().min()) > -1e-5 * S and float(resid.diagonal().sum()) < float(Kd.diagonal().sum())
        assert max(e_d, e_r, e_g) < 1e-5, (kind, d, e_d, e_r, e_g)


@pytest.mark.parametrize("kind", ["rbf", "matern12", "matern52"])
def test_kernel_api_native_branch(kind, dev):
    """The kernel's call builds a FusedKernelLinearOperator of kind "ng"; K V, K and the diagonals match ``ng_dense`` of the float64 twin; gradients of
    the raw lengthscales and raw outputscales through a product and through to_dense match float64 autograd; a ScaleKernel base and a float64 model
    land on the dense branch."""
    import gpytorch_amd as g
    from gpytorch_amd.kernels import ng_dense
    from gpytorch_amd.operators import DenseLinearOperator, FusedKernelLinearOperator, to_dense

    d, r, n, m = 5, 3, 400, 233
    gen = torch.Generator().manual_seed(21 + FAMILIES.index(kind))
    x, x2, ls, sigma = _cloud(gen, n, d, "lattice"), _cloud(gen, m, d), _ls(gen, d), _sigma(gen, r)
    base = _base(g, kind, ard_num_dims=d)
    kern = _ng(g, base, d, r).to(dev)
    base.lengthscale, kern.outputscale = ls.float().reshape(1, d), sigma.float()
    twin_base = _base(g, kind, ard_num_dims=d).double()
    twin = _ng(g, twin_base, d, r).double()
    twin_base.lengthscale, twin.outputscale = base.lengthscale.detach().double().cpu(), kern.outputscale.detach().double().cpu()
    lsv, sgv = twin_base.lengthscale.detach().reshape(-1), twin.outputscale.detach()
    S = float(ng_norm(sgv, d))
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "ng" and op.shape == (n, n)
    with torch.no_grad():
        Kref = ng_dense(twin_base, x, x, sgv, r)
        assert rel_err(Kref, ng_cov(kind, x, x, lsv, sgv)) < 1e-10
        assert rel_err(op.to_dense(), Kref) < 1e-5
        assert rel_err(kern(xd, x2d).to_dense(), ng_dense(twin_base, x, x2, sgv, r)) < 1e-5
        V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
        ref = Kref @ V.double()
        out = (op @ V.to(dev)).double().cpu()
        assert _col_err(out, ref) < 2e-5
        assert torch.allclose(kern(xd, diag=True).cpu(), torch.full((n,), S), rtol=1e-6)              # S, no launch
        assert rel_err(kern(xd[:m], x2d, diag=True), ng_dense(twin_base, x[:m], x2, sgv, r, diag=True)) < 1e-5   # two inputs: the dense branch
        assert rel_err(op.diagonal(), torch.full((n,), S)) < 1e-6
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    want_m = torch.autograd.grad((U.double() * (ng_dense(twin_base, x, x, twin.outputscale, r) @ V.double())).sum(), [twin_base.raw_lengthscale, twin.raw_outputscale])
    want_d = torch.autograd.grad((W.double() * ng_dense(twin_base, x, x, twin.outputscale, r)).sum(), [twin_base.raw_lengthscale, twin.raw_outputscale])
    for how, want in (("matmul", want_m), ("dense", want_d)):
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        for a, b, what in zip((base.raw_lengthscale.grad, kern.raw_outputscale.grad), want, ("raw_lengthscale", "raw_outputscale")):
            e = float((a.double().cpu().reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max())
            print("api grad", kind, how, what, e)
            assert e < 2e-3, (how, what, a, b)
    # outside the rule: the dense branch
    sk = g.kernels.ScaleKernel(_base(g, kind, ard_num_dims=d))
    ks = _ng(g, sk, d, r).to(dev)
    sk.base_kernel.lengthscale, sk.outputscale, ks.outputscale = ls.float().reshape(1, d), 1.7, sigma.float()
    assert isinstance(ks(xd), DenseLinearOperator)
    k64 = _ng(g, _base(g, kind, ard_num_dims=d), d, r).to(dev).double()
    k64.base_kernel.lengthscale, k64.outputscale = lsv.reshape(1, d), sgv
    o64 = k64(x.to(dev))
    assert isinstance(o64, DenseLinearOperator) and rel_err(to_dense(o64), Kref) < 1e-10


def test_matrix_free_at_size(dev):
    """n = 40 000, d = 6, R = 3, eleven columns: the device memory ``op @ V`` adds at its peak stays below ONE n x n float32 matrix (6.4 GB; the
    reference's d x n x m tensor, R power sums and R + 1 polynomials are ten of them); 64 rows are checked against the closed form."""
    import gpytorch_amd as g

    n, t, d, r = 40_000, 11, 6, 3
    gen = torch.Generator().manual_seed(5)
    x, ls, sigma = _cloud(gen, n, d), _ls(gen, d), _sigma(gen, r)
    V = torch.randn(n, t, generator=gen, dtype=torch.float64).float()
    base = _base(g, "matern52", ard_num_dims=d)
    kern = _ng(g, base, d, r).to(dev)
    base.lengthscale, kern.outputscale = ls.float().reshape(1, d), sigma.float()
    xd, Vd = x.float().to(dev), V.to(dev)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = kern(xd) @ Vd
        torch.cuda.synchronize()
        added = torch.cuda.max_memory_allocated() - before
    print("peak bytes added", added, "dense K", 4 * n * n)
    assert added < 4 * n * n, added
    rows = torch.randint(0, n, (64,), generator=gen)
    lsv, sgv = base.lengthscale.detach().double().cpu().reshape(-1), kern.outputscale.detach().double().cpu()
    ref = ng_cov("matern52", x[rows], x, lsv, sgv) @ V.double()
    err = _col_err(out[rows.to(dev)].double().cpu(), ref)
    print("at size", err)
    assert err < 2e-5, err


MODEL_N, MODEL_D, MODEL_R, MODEL_LS, MODEL_SIGMA, MODEL_NOISE = 600, 4, 3, (0.2, 0.25, 0.3, 0.35), (0.8, 0.3, 0.1), 0.1


def _gp_class(g):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = _ng(g, g.kernels.MaternKernel(nu=2.5, ard_num_dims=MODEL_D), MODEL_D, MODEL_R)

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _set_model(m, lik):
    m.covar_module.base_kernel.lengthscale = torch.tensor([MODEL_LS])
    m.covar_module.outputscale = torch.tensor(MODEL_SIGMA)
    lik.noise = MODEL_NOISE


def test_gp_mll_cholesky_and_bbmm(dev):
    """NewtonGirardAdditiveKernel(Matern-5/2, ARD, R = 3) + Gaussian noise, n = 600, d = 4: the marginal log likelihood and all hyper-parameter
    gradients (d raw lengthscales, R raw outputscales, the noise) on the Cholesky branch and on the BBMM branch against dense float64 autograd, with
    the settings and bounds of tests/test_gpu_additive.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    n, d = MODEL_N, MODEL_D
    X, y = make_data(n, d)
    X, y = _f32(X), _f32(y)
    ls = torch.tensor(MODEL_LS, dtype=torch.float64, requires_grad=True)
    sg = torch.tensor(MODEL_SIGMA, dtype=torch.float64, requires_grad=True)
    nz = torch.tensor(MODEL_NOISE, dtype=torch.float64, requires_grad=True)
    ref = OG.dense_log_prob(ng_cov("matern52", X, X, ls, sg) + nz * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, [ls, sg, nz])
    M = _gp_class(g)
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        op = m.covar_module(m.train_inputs[0])
        assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "ng"
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
        sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731   (d softplus / d raw at the value v)
        got = torch.tensor([float(v) for v in m.covar_module.base_kernel.raw_lengthscale.grad.reshape(-1)]
                           + [float(v) for v in m.covar_module.raw_outputscale.grad.reshape(-1)] + [float(lik.noise_covar.raw_noise.grad.sum())], dtype=torch.float64)
        want = torch.tensor([float(gref[0][q]) * sp(MODEL_LS[q]) for q in range(d)] + [float(gref[1][k]) * sp(MODEL_SIGMA[k]) for k in range(MODEL_R)]
                            + [float(gref[2]) * sp(MODEL_NOISE - 1e-4)], dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("mll", branch, e_v, e_g, got, want)
        assert e_v < tol_v, (branch, float(val), float(ref))
        assert e_g < tol_g, (branch, got, want)


def test_gp_posterior_fast_pred_var_and_fantasy(dev):
    """Posterior mean and variance of the same model against the dense float64 posterior, exact and with ``fast_pred_var`` (LOVE), then a fantasy
    model on 40 more observations against the dense posterior of the enlarged data set: settings and bounds of
    tests/test_gpu_additive.py::test_gp_posterior_fast_pred_var_and_fantasy (exact variances at ``eval_cg_tolerance(1e-6)``)."""
    import gpytorch_amd as g

    n, nf, ns, d = MODEL_N, 40, 150, MODEL_D
    X, y = make_data(n + nf + ns, d)
    X, y = _f32(X), _f32(y)
    Xt, yt, Xf, yf, Xs = X[:n], y[:n], X[n : n + nf], y[n : n + nf], X[n + nf :]
    ls, sg = torch.tensor(MODEL_LS, dtype=torch.float64), torch.tensor(MODEL_SIGMA, dtype=torch.float64)
    prior = float(ng_norm(sg, d))

    def dense_posterior(Xa, ya):
        Lc = torch.linalg.cholesky(ng_cov("matern52", Xa, Xa, ls, sg) + MODEL_NOISE * torch.eye(Xa.shape[0], dtype=torch.float64))
        Ks = ng_cov("matern52", Xs, Xa, ls, sg)
        mu = (Ks @ torch.cholesky_solve(ya.unsqueeze(-1), Lc)).squeeze(-1)
        return mu, prior + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)

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
                S.max_root_decomposition_size(n):
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
