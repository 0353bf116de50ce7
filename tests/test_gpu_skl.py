"""GPU: Gaussian inputs under the symmetrized KL divergence as ONE matrix-free operator (``GPAMD_SKL``; csrc/kv_directskl.hpp, csrc/kv_grad_skl.hpp,
``kernels.GaussianSymmetrizedKLKernel``).

Oracle: tests/skl_ref.py, a float64 restatement written from the formulas and pinned to the reference's own outputs (tests/test_skl_cpu.py).  Inputs:
mu uniform in [0, 1]^d, log sigma^2 uniform in [-3, -1], lengthscale = d, everything rounded through float32 before the oracle sees it.  Per d ONE pair of
clouds (300 and 4 j tiles + 6 = 518 points) and ONE float64 covariance, of which every shape is a leading block; the precondition -- between 5 % and
95 % of the covariances lie in (0.05, 0.95) -- is asserted on it.  Bounds, the project's:
  * K V: per column, relative to max |K| |V|, 2e-5;   entries of K, max-normalised: 1e-5, the diagonal exactly 1.0;
  * derivative pass: G0, G1 and the per-point gradients (max-normalised, as tests/test_gpu_gibbs.py measures its per-point gradient) 2e-3;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3."""
import functools
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from tests.skl_ref import skl_grad_sums, skl_K
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 3, 6)          # both ends of width 4 (d = 1) and width 20 (d = 6, with 5), the first d of width 12 and one inside it
ROWS, JTILE = 128, 128       # rows of a workgroup below 16 384 output rows (4 waves x one 32-row tile); the j tile staged in LDS
N, M = 300, 4 * JTILE + 6
SHAPES = [(1, 1), (7, 5), (ROWS + 1, JTILE + 1), (N, M)]


def _cloud(gen, n, d, offset=0.0):
    x = torch.cat([offset + torch.rand(n, d, generator=gen, dtype=torch.float64), -3.0 + 2.0 * torch.rand(n, d, generator=gen, dtype=torch.float64)], -1)
    return x.float().double()   # values the float32 kernels receive exactly


@functools.lru_cache(maxsize=None)
def _case(d, offset=0.0):
    """(X1 [N, 2 d], X2 [M, 2 d], K [N, M]) in float64, made once per d and left unchanged."""
    gen = torch.Generator().manual_seed(40 + d)
    X1, X2 = _cloud(gen, N, d, offset), _cloud(gen, M, d, offset)
    K = skl_K(X1, X2, float(d))
    share = float(((K > 0.05) & (K < 0.95)).double().mean())
    assert 0.05 <= share <= 0.95, (d, share)
    return X1, X2, K


def _prep(B, X, d, shift, dev):
    return B.prep_points("skl", X.float().to(dev), torch.tensor([[float(d)]], device=dev), shift.float().to(dev))


@pytest.mark.parametrize("d,n,m,t,offset", [(d, n, m, t, 0.0) for d in DIMS for n, m in SHAPES for t in (1, 32, 33, 65)] + [(3, N, M, 33, 1000.0)])
def test_kv_matches_restatement(d, n, m, t, offset, dev):
    """Every width, fewer rows than a tile and one more than a row block / a j tile, the 32-column tile, its extra column and the next group; last,
    a cloud whose means lie 1000 from the origin."""
    from gpytorch_amd import backend as B

    X1, X2, K = _case(d, offset)
    V = torch.randn(m, t, generator=torch.Generator().manual_seed(t), dtype=torch.float64).float()
    shift = X1[:n, :d].mean(0)
    p1, p2 = _prep(B, X1[:n], d, shift, dev), _prep(B, X2[:m], d, shift, dev)
    assert p1.kind == "skl" and p1.dp == p1.d == {1: 4, 2: 12, 3: 12, 6: 20}[d] and B.kv_flags(p1, p2, t) == B.KV_SPLIT
    out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
    Kb = K[:n, :m]
    err = float(((out - Kb @ V.double()).abs().max(0).values / (Kb.abs() @ V.double().abs()).max(0).values).max())
    print("kv", (d, n, m, t, offset), err)
    assert err < 2e-5, ((d, n, m, t, offset), err)


@pytest.mark.parametrize("d", DIMS)
def test_entries_through_the_kernel_api(d, dev):
    """Dense block, rows, elementwise diagonal, transpose, point slices and ``+ diag`` of the operator the kernel returns; the diagonal is exactly 1."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelAddedDiagLinearOperator, FusedKernelLinearOperator

    X1, X2, K = _case(d)
    kern = g.kernels.GaussianSymmetrizedKLKernel().to(dev)
    kern.lengthscale = float(d)
    x1, x2 = X1.float().to(dev), X2.float().to(dev)
    idx = torch.tensor([0, N - 1, N // 2], device=dev)
    with torch.no_grad():
        op, sq = kern(x1, x2), kern(x1)
        assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "skl" and op.shape == (N, M)
        Ksq = skl_K(X1, X1, float(d))
        errs = [rel_err(op.to_dense(), K), rel_err(op.rows(idx), K[idx.cpu()]), rel_err(op[:N, :N].diagonal(), K[:N, :N].diagonal()),
                rel_err(op.t().to_dense(), K.t()), rel_err(op[5:40, 3:77].to_dense(), K[5:40, 3:77]), rel_err(sq.to_dense(), Ksq)]
        added = sq.add_diagonal(torch.tensor([0.3], device=dev))
        assert isinstance(added, FusedKernelAddedDiagLinearOperator)
        errs.append(rel_err(added.to_dense(), Ksq + 0.3 * torch.eye(N, dtype=torch.float64)))
        ones = torch.ones(N, device=dev)
        assert torch.equal(sq.diagonal(), ones) and torch.equal(kern(x1, diag=True), ones) and torch.equal(sq.to_dense().diagonal(), ones)
    print("entries", d, errs)
    assert max(errs) < 1e-5, (d, errs)


@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("square", [True, False])
@pytest.mark.parametrize("d", DIMS)
def test_derivative_pass(d, square, t, dev):
    """``backend.kv_grad_skl`` against the float64 closed form with W = L R^T: G0, G1 and the gradients with respect to mu and a of every point of both
    clouds (the second cloud's from the exchanged call); two calls return the same bits."""
    from gpytorch_amd import backend as B

    X1, X2, _ = _case(d)
    X2 = X1 if square else X2
    n, m = X1.shape[0], X2.shape[0]
    gen = torch.Generator().manual_seed(7 + t)
    Lm, Rm = (torch.randn(k, t, generator=gen, dtype=torch.float64).float() for k in (n, m))
    W = Lm.double() @ Rm.double().t()
    g0, g1, gm1, ga1 = skl_grad_sums(X1, X2, float(d), W)
    _, _, gm2, ga2 = skl_grad_sums(X2, X1, float(d), W.t())
    shift = X1[:, :d].mean(0)
    p1 = _prep(B, X1, d, shift, dev)
    p2 = p1 if square else _prep(B, X2, d, shift, dev)
    lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
    s, rm1, ra1 = B.kv_grad_skl(p1, p2, lt, rt)
    s2, rm2, ra2 = B.kv_grad_skl(p2, p1, rt, lt)
    sb, rm1b, ra1b = B.kv_grad_skl(p1, p2, lt, rt)
    assert torch.equal(s, sb) and torch.equal(rm1, rm1b) and torch.equal(ra1, ra1b)      # no atomics: the same bits
    assert rm1.shape == ra1.shape == (n, d) and rm2.shape == ra2.shape == (m, d)
    want = torch.stack([g0, g1])
    errs = [rel_err(s, want), rel_err(s2, want), rel_err(rm1, gm1), rel_err(ra1, ga1), rel_err(rm2, gm2), rel_err(ra2, ga2)]
    print("grad", (d, square, t), errs)
    assert max(errs) < 2e-3, ((d, square, t), errs)


MODEL_D, MODEL_OS, MODEL_NOISE, NTEST = 2, 1.0, 0.5, 50   # (the kernel is not positive definite: smallest eigenvalue of k(Z, Z) -0.18; the noise covers it)


def _model_data():
    gen = torch.Generator().manual_seed(5)
    Z = _cloud(gen, N + NTEST, MODEL_D)
    y = make_data(N + NTEST, MODEL_D)[1].float().double() + torch.sin(3.0 * Z[:, 0])
    return Z, y


def _gp(g, Z, y, dev):
    class M(g.models.ExactGP):
        """The training points' log sigma^2 is a learned tensor: in training mode it replaces the variance columns of the inputs."""

        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(g.kernels.GaussianSymmetrizedKLKernel())
            self.logvar = torch.nn.Parameter(x[:, MODEL_D:].clone())

        def forward(self, x):
            z = torch.cat([x[:, :MODEL_D], self.logvar], -1) if self.training else x
            return g.distributions.MultivariateNormal(self.mean_module(z), self.covar_module(z))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = M(Z.float().to(dev), y.float().to(dev), lik).to(dev)
    m.covar_module.outputscale, m.covar_module.base_kernel.lengthscale, lik.noise = MODEL_OS, float(MODEL_D), MODEL_NOISE
    return m, lik


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
def test_gp_mll_with_a_learned_per_point_variance(branch, dev):
    """ScaleKernel(GaussianSymmetrizedKLKernel()) + Gaussian noise, n = 300, d = 2: the marginal log likelihood and its gradients with respect to the
    lengthscale, the outputscale, the noise AND the learned log sigma^2 of every training point, against a dense float64 Cholesky evaluation of
    ``skl_dense`` under autograd.  Measured as tests/test_gpu_gibbs.py measures its model: the value, and ONE vector of the gradients of all learned
    parameters, norm-relative.  The per-point part ALONE is asserted on the Cholesky branch, where it is exact (2.2e-6 on an MI355X); on the BBMM
    branch it is printed only: every component is a 300-probe trace estimate of its own and that part alone is 0.29 off (the whole vector 0.06)."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    Z, y = _model_data()
    Z, y = Z[:N], y[:N]
    ls, os_, nz = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (float(MODEL_D), MODEL_OS, MODEL_NOISE))
    logvar = Z[:, MODEL_D:].clone().requires_grad_(True)
    z64 = torch.cat([Z[:, :MODEL_D], logvar], -1)
    Khat = os_ * g.kernels.skl_dense(z64, z64, ls) + nz * torch.eye(N, dtype=torch.float64)
    assert float(torch.linalg.eigvalsh(Khat.detach()).min()) >= MODEL_NOISE / 2
    ref = OG.dense_log_prob(Khat, y) / N
    gref = torch.autograd.grad(ref, [ls, os_, nz, logvar])
    sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731   (d softplus / d raw at the value v)
    want = torch.stack([gref[0] * sp(float(MODEL_D)), gref[1] * sp(MODEL_OS), gref[2] * sp(MODEL_NOISE - 1e-4)])

    m, lik = _gp(g, Z, y, dev)
    m.train()
    lik.train()
    op = m.covar_module(torch.cat([m.train_inputs[0][:, :MODEL_D], m.logvar], -1))
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "skl" and op.x1.requires_grad
    S = g.settings
    with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(300), \
            S.max_preconditioner_size(15), S.deterministic_probes(True), S.max_lanczos_quadrature_iterations(100):
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        val = g.ExactMarginalLogLikelihood(lik, m)(m(m.train_inputs[0]), m.train_targets)
        val.backward()
        S.deterministic_probes.reset()
    got = torch.stack([p.grad.detach().double().cpu().reshape(-1).sum() for p in
                       (m.covar_module.base_kernel.raw_lengthscale, m.covar_module.raw_outputscale, lik.noise_covar.raw_noise)])
    tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
    e_v = abs(float(val) - float(ref)) / max(1.0, abs(float(ref)))
    gx = m.logvar.grad.double().cpu()
    got, want = torch.cat([got, gx.reshape(-1)]), torch.cat([want, gref[3].reshape(-1)])
    e_g, e_x = float((got - want).norm() / want.norm()), float((gx - gref[3]).norm() / gref[3].norm())
    print("mll", branch, e_v, e_g, e_x)
    assert e_v < tol_v and e_g < tol_g and (branch == "bbmm" or e_x < tol_g), (branch, e_v, e_g, e_x)


def test_gp_posterior(dev):
    """Posterior mean and variance at inputs with given variances against the dense float64 posterior."""
    import gpytorch_amd as g

    Z, y = _model_data()
    Zt, yt, Zs = Z[:N], y[:N], Z[N:]
    cov = lambda A, Bm: MODEL_OS * skl_K(A, Bm, float(MODEL_D))  # noqa: E731
    Lc = torch.linalg.cholesky(cov(Zt, Zt) + MODEL_NOISE * torch.eye(N, dtype=torch.float64))
    Ks = cov(Zs, Zt)
    mu_ref = (Ks @ torch.cholesky_solve(yt.unsqueeze(-1), Lc)).squeeze(-1)
    var_ref = MODEL_OS + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)
    m, lik = _gp(g, Zt, yt, dev)
    m.eval()
    lik.eval()
    S = g.settings
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(False), S.eval_cg_tolerance(1e-6):
        warnings.simplefilter("ignore")
        pred = lik(m(Zs.float().to(dev)))
    e_mu, e_var = rel_err(pred.mean, mu_ref), rel_err(pred.variance, var_ref)
    print("posterior", e_mu, e_var)
    assert e_mu < 2e-3 and e_var < 2e-3, (e_mu, e_var)
