"""What the two estimator settings of tests/test_gpu_piecewise.py's model tests rest on (n = 3000, d = 2, lengthscale 0.3, outputscale 1.3, noise 0.1,
the data of tests/util.make_data), for the piecewise-polynomial family q = 0 .. 3 and, as yardsticks, Matern-1/2 and Matern-5/2:
  * the BBMM marginal log likelihood against dense float64 by number of probes and of Lanczos quadrature nodes
    (settings.max_lanczos_quadrature_iterations; no preconditioner, cg_tolerance 1e-5, deterministic probes);
  * the posterior variance against dense float64 by LOVE rank (settings.max_root_decomposition_size under fast_pred_var) and without LOVE.
python scripts/pp_estimator_settings.py [out.json]  -> profiles/pp_estimator_settings.json"""
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402
from oracle import exact_gp as OG  # noqa: E402
from oracle import kernels as OK  # noqa: E402
from tests.piecewise_ref import pp_cov  # noqa: E402
from tests.util import make_data, rel_err  # noqa: E402

warnings.simplefilter("ignore")
path = sys.argv[1] if len(sys.argv) > 1 else "profiles/pp_estimator_settings.json"
dev = torch.device("cuda:0")
n, ns, d = 3000, 200, 2
X, y = make_data(n + ns, d)
X, y = X.float().double(), y.float().double()
Xt, yt, Xs = X[:n], y[:n], X[n:]
S = g.settings
LS = torch.tensor([0.3], dtype=torch.float64)


def matern(kind):
    return lambda a, b: OK.kernel_matrix(kind, a, b, 0.3, 1.0, x1_eq_x2=False, direct=True)


FAMILIES = [(f"pp_q{q}", (lambda q=q: g.kernels.PiecewisePolynomialKernel(q=q)), (lambda a, b, q=q: pp_cov(a, b, LS, q))) for q in range(4)]
FAMILIES += [("matern12", lambda: g.kernels.MaternKernel(nu=0.5), matern("matern12")), ("matern52", lambda: g.kernels.MaternKernel(nu=2.5), matern("matern52"))]


def model(make):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(make())

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = M(Xt.float().to(dev), yt.float().to(dev), lik).to(dev)
    m.covar_module.base_kernel.lengthscale, m.covar_module.outputscale, lik.noise = 0.3, 1.3, 0.1
    return m, lik


out = {"n": n, "d": d, "lengthscale": 0.3, "outputscale": 1.3, "noise": 0.1, "device": torch.cuda.get_device_name(0), "mll": [], "posterior_variance": []}
for name, make, dense in FAMILIES:
    Kh = 1.3 * dense(Xt, Xt) + 0.1 * torch.eye(n, dtype=torch.float64)
    ref = float(OG.dense_log_prob(Kh, yt) / n)
    for probes, nodes, seed in [(300, 20, 0), (300, 20, 1), (3000, 20, 0), (300, 100, 0), (3000, 100, 0)]:
        m, lik = model(make)
        m.train(), lik.train()
        mll = g.ExactMarginalLogLikelihood(lik, m)
        with S.max_cholesky_size(0), S.cg_tolerance(1e-5), S.num_trace_samples(probes), S.max_preconditioner_size(0), S.deterministic_probes(True), \
                S.max_lanczos_quadrature_iterations(nodes), torch.no_grad():
            torch.manual_seed(seed)
            val = float(mll(m(m.train_inputs[0]), m.train_targets))
        S.deterministic_probes.reset()
        rec = dict(family=name, probes=probes, quadrature_nodes=nodes, seed=seed, value=val, dense_float64=ref, error=abs(val - ref) / max(1.0, abs(ref)))
        print(json.dumps(rec), flush=True)
        out["mll"].append(rec)
    Lc = torch.linalg.cholesky(Kh)
    Ks = 1.3 * dense(Xs, Xt)
    var_ref = 1.3 + 0.1 - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)
    for rank, fast in [(100, True), (400, True), (1500, True), (100, False)]:
        m, lik = model(make)
        m.eval(), lik.eval()
        torch.manual_seed(1)
        with torch.no_grad(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4), S.max_root_decomposition_size(rank):
            var = lik(m(Xs.float().to(dev))).variance.double().cpu()
        rec = dict(family=name, fast_pred_var=fast, love_rank=rank if fast else None, max_rel_error=rel_err(var, var_ref),
                   dense_variance_range=[float(var_ref.min()), float(var_ref.max())])
        print(json.dumps(rec), flush=True)
        out["posterior_variance"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
