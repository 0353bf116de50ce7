"""Device tests of the linear model of coregionalisation (csrc/kv_lcm.hpp, gpytorch_amd/lcm.py) against tests/lcm_ref.py in float64.

Bounds: the product per column 2e-5 of the largest entry of sum_q theta_q K_q |W_q| (the bound of tests/test_gpu_product_structure.py and
test_gpu_hamming.py for this arithmetic, on a scale that cancellation between members cannot shrink); operator surfaces 1e-5 max-normalised; the
model 2e-4 / 3e-3 (value / gradients) on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch, posterior 2e-3 -- those of the Kronecker and Hamming
model tests."""
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from tests.lcm_ref import lcm_matrix, member_k, task_covar

pytestmark = pytest.mark.gpu

NUS = (None, 0.5, 1.5, 2.5)
KINDS = ("rbf", "matern12", "matern32", "matern52")


def _members(d, Q, T, seed):
    """Q members over all four families in turn: member 0 with d lengthscales and an outputscale, lengthscales 0.3 .. 2."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for q in range(Q):
        ls = torch.linspace(0.3, 2.0, d, dtype=torch.float64) if q == 0 else torch.tensor([0.3 + 1.7 * (q / 3.0)], dtype=torch.float64)
        out.append((q % 4, ls, 1.7 if q == 0 else 1.0, task_covar(torch.randn(T, 1, generator=gen), torch.rand(T, generator=gen) + 0.2)))
    return out


# n, m (None: the same cloud), d, Q, T, probes  ->  T t = 2, 30, 32, 33 (a second launch group), 40; (2000, 1200): the planner splits the contracted index into
# two chunks (640 + a ragged 560) once 16 row blocks make the split worth a hundredth of the chip, so two slabs are written and summed
@pytest.mark.parametrize("n,m,d,Q,T,t", [(1, None, 1, 1, 2, 1), (127, 129, 3, 2, 3, 10), (129, 517, 4, 4, 8, 4), (300, 1, 3, 2, 3, 11), (300, None, 3, 4, 8, 5),
                                         (2000, 1200, 3, 3, 3, 2)])
def test_product_against_float64(dev, n, m, d, Q, T, t):
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(n + (m or 0))
    x1 = torch.rand(n, d, generator=gen, dtype=torch.float64)
    x2 = x1 if m is None else torch.rand(m, d, generator=gen, dtype=torch.float64)
    mm = x2.shape[0]
    V = torch.randn(mm * T, t, generator=gen, dtype=torch.float64)
    mem = _members(d, Q, T, 3)
    ref = lcm_matrix(x1, x2, [(NUS[f], ls, th, bq) for f, ls, th, bq in mem]) @ V
    eye = torch.eye(T, dtype=torch.float64)
    scale = sum(torch.kron(th * member_k(NUS[f], ls, x1, x2), eye) @ (torch.kron(torch.eye(mm, dtype=torch.float64), bq) @ V).abs() for f, ls, th, bq in mem)
    shift = x1.mean(0)
    x1c = B.lcm_points(x1.float().to(dev), shift)
    x2c = x1c if m is None else B.lcm_points(x2.float().to(dev), shift)
    block = B.lcm_block([KINDS[f] for f, *_ in mem], [ls for _, ls, _, _ in mem], [(th * bq).to(dev) for _, _, th, bq in mem], d)
    vt = B.to_probe_major(V.float().to(dev))
    S = B.LcmPlan(x1c, x2c, block, d, T, t).S
    assert S >= 2 if mm == 1200 else S == 1, S
    got = B.lcm_kv(x1c, x2c, block, d, T, vt)
    again = B.lcm_kv(x1c, x2c, block, d, T, vt)
    assert torch.equal(got[:, : n * T], again[:, : n * T])
    err = (B.from_probe_major(got, n * T).double().cpu() - ref).abs().amax(0) / scale.amax(0)
    print("lcm product", (n, m, d, Q, T, t), float(err.max()))
    assert float(err.max()) < 2e-5, err


def _model(g, dev, X, Y, T=2):
    class M(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.mean_module = g.means.MultitaskMean(g.means.ZeroMean(), num_tasks=T)
            self.covar_module = g.kernels.LCMKernel([g.kernels.ScaleKernel(g.kernels.RBFKernel(ard_num_dims=2)), g.kernels.MaternKernel(nu=1.5)], num_tasks=T)

        def forward(self, x):
            return g.distributions.MultitaskMultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.MultitaskGaussianLikelihood(num_tasks=T, has_global_noise=False).to(dev)
    m = M(X.float().to(dev), Y.float().to(dev), lik).to(dev)
    a, b = m.covar_module.covar_module_list
    a.data_covar_module.base_kernel.lengthscale = torch.tensor([[0.5, 0.9]])
    a.data_covar_module.outputscale = 1.4
    b.data_covar_module.lengthscale = 0.7
    gen = torch.Generator().manual_seed(5)
    for mt in (a, b):
        with torch.no_grad():
            mt.task_covar_module.covar_factor.copy_(torch.randn(T, 1, generator=gen))
        mt.task_covar_module.var = torch.rand(T, generator=gen) + 0.3
    lik.task_noises = torch.tensor([0.05, 0.08])
    return m, lik


def _raw(m, lik):
    a, b = m.covar_module.covar_module_list
    return [a.data_covar_module.base_kernel.raw_lengthscale, a.data_covar_module.raw_outputscale, a.task_covar_module.covar_factor, a.task_covar_module.raw_var,
            b.data_covar_module.raw_lengthscale, b.task_covar_module.covar_factor, b.task_covar_module.raw_var, lik.raw_task_noises]


def _ref_khat(raw, x1, x2, T=2, noise=True):
    """The model's covariance from float64 copies of its raw parameters (softplus constraints; the task noise is bounded below by 1e-4)."""
    sp = torch.nn.functional.softplus
    ls0, os0, f0, v0, ls1, f1, v1, tn = raw
    K = lcm_matrix(x1, x2, [(None, sp(ls0).reshape(-1), sp(os0), task_covar(f0, sp(v0))), (1.5, sp(ls1).reshape(-1), 1.0, task_covar(f1, sp(v1)))])
    return K + torch.diag((sp(tn) + 1e-4).repeat(x1.shape[0])) if noise else K


def _data(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 2, generator=gen, dtype=torch.float64)
    Y = torch.stack([torch.sin(5 * X[:, 0]) + X[:, 1], torch.cos(4 * X[:, 0] * X[:, 1])], -1) + 0.1 * torch.randn(n, 2, generator=gen, dtype=torch.float64)
    return X, Y


def test_operator_surfaces(dev):
    """to_dense, diagonal and one preconditioner row of the fused operator at n = 129, max-normalised 1e-5."""
    import gpytorch_amd as g
    from gpytorch_amd.lcm import LCMFusedAddedDiagLinearOperator, LCMFusedLinearOperator

    X, Y = _data(129)
    m, lik = _model(g, dev, X, Y)
    op = m.covar_module(m.train_inputs[0])
    assert isinstance(op, LCMFusedLinearOperator) and op.shape == (258, 258)
    assert isinstance(lik(m.train()(m.train_inputs[0])).lazy_covariance_matrix, LCMFusedAddedDiagLinearOperator)
    ref = _ref_khat([p.detach().double().cpu() for p in _raw(m, lik)], X, X, noise=False)
    with torch.no_grad():
        for got, want in ((op.to_dense(), ref), (op.diagonal(), ref.diagonal()), (op._row(torch.tensor(101)), ref[101])):
            assert float((got.double().cpu() - want).abs().max() / want.abs().max()) < 1e-5


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
def test_gp_mll_and_gradients(dev, branch):
    """n = 150, T = 2, Q = 2, d = 2: the marginal log likelihood and the gradient of every raw parameter against float64 autograd through the dense
    reference and a Cholesky factorisation.  Settings and bounds are those of tests/test_gpu_hamming.py::test_gp_mll_cholesky_and_bbmm
    (300 deterministic probes on the BBMM branch).  Measured with the library's default of 10 probes instead, the value deviates by 1.3e-2 and the
    gradients by 2.9e-2; the Kronecker ``MultitaskKernel`` model at the same shape by 1.4e-2 / 5.7e-2: the variance of a 10-probe log-determinant."""
    import gpytorch_amd as g

    n = 150
    X, Y = _data(n)
    m, lik = _model(g, dev, X, Y)
    raw64 = [p.detach().double().cpu().requires_grad_(True) for p in _raw(m, lik)]
    ref = OG.dense_log_prob(_ref_khat(raw64, X, X), Y.reshape(-1)) / (n * 2)
    want = torch.cat([gr.reshape(-1) for gr in torch.autograd.grad(ref, raw64)])
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
    got = torch.cat([p.grad.reshape(-1).double().cpu() for p in _raw(m, lik)])
    tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
    e_v, e_g = abs(float(val.detach()) - float(ref.detach())) / max(1.0, abs(float(ref.detach()))), float((got - want).norm() / want.norm())
    print("lcm mll", branch, e_v, e_g, got, want)
    assert e_v < tol_v, (branch, float(val), float(ref))
    assert e_g < tol_g, (branch, got, want)


def test_gp_posterior(dev):
    """Posterior mean and variance of the same model on 20 test points against the dense float64 posterior, 2e-3."""
    import gpytorch_amd as g

    n, ns = 150, 20
    X, Y = _data(n + ns, seed=1)
    Xt, Yt, Xs = X[:n], Y[:n], X[n:]
    m, lik = _model(g, dev, Xt, Yt)
    raw = [p.detach().double().cpu() for p in _raw(m, lik)]
    Lc = torch.linalg.cholesky(_ref_khat(raw, Xt, Xt))
    Ks = _ref_khat(raw, Xs, Xt, noise=False)
    mu_ref = (Ks @ torch.cholesky_solve(Yt.reshape(-1, 1), Lc)).reshape(ns, 2)
    var_ref = (_ref_khat(raw, Xs, Xs).diagonal() - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)).reshape(ns, 2)
    m.eval()
    lik.eval()
    S = g.settings
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(False), S.eval_cg_tolerance(1e-6):
        warnings.simplefilter("ignore")
        pred = lik(m(Xs.float().to(dev)))
        mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
    e_mu, e_var = float((mu - mu_ref).norm() / mu_ref.norm()), float((var - var_ref).norm() / var_ref.norm())
    print("lcm posterior", e_mu, e_var)
    assert e_mu < 2e-3 and e_var < 2e-3, (e_mu, e_var)
