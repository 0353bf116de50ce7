"""GPU: the RBF kernel with first- and second-derivative observations as ONE matrix-free operator (csrc/kv_rbfgradgrad.hpp,
``derivative.RBFGradGradFusedLinearOperator``, ``kernels.RBFKernelGradGrad`` / ``rbfgradgrad_native``).

Oracle of every test: tests/rbfgradgrad_ref.py, a float64 restatement written from the Hermite formula as loops over the components.  Inputs are
uniform in [0, 1]^d and lengthscales lie in 0.3 .. 0.4 (every one different under ARD), the clouds of tests/test_gpu_matern52grad.py; the product
tests assert that at least half of the pair covariances k lie in (0.05, 0.95), so neither a missing block nor a swapped dimension can pass.  Bounds:
  * K V: per column, relative to the column maximum of |K| |V|, 2e-5 (the project's K V bound, tests/test_gpu_product.py);
  * entries of K (dense, rows, diagonal, slices, transpose, + diag), max-normalised: 1e-5;
  * hyper-gradients of sum_c l_c^T K r_c: 2e-3, the project's bound for every family;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3 (mean), 2e-3 / 5e-2
    (variance without / with fast_pred_var); fantasy model 2e-3 -- the bounds of tests/test_gpu_matern52grad.py.  Second-derivative entries of K
    scale as 3 / l^4 (117 at l = 0.4 against 6 for the first derivatives and 1 for the value), so the per-task noises grow with the order
    (0.05, 0.3, 0.3, 5, 5: 3..4 % of the task's prior variance each); the MLL tests assert, as a condition on the inputs, that float32 dense torch
    Cholesky on the host reproduces the float64 MLL to better than a quarter of the asserted tolerance."""
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from tests import rbfgradgrad_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROW_TILE, J_TILE = 1024, 256                     # csrc/kv_rbfgrad.hpp KRG_BM, KRG_BN
WIDEST_T = {1: 4, 2: 4, 3: 4, 4: 2}              # csrc/kv_rbfgradgrad.hpp krg2_max_t(d)
# (n, m); m = 0: the same cloud.  One below / at / one above the row tile and the j tile (257 points: two split-j slabs), a tiny pair, one point
KV_SIZES = [(1, 0), (7, 5), (ROW_TILE - 1, J_TILE - 1), (ROW_TILE, J_TILE), (ROW_TILE + 1, J_TILE + 1), (300, 4 * J_TILE + 6)]


# The seeds are those of tests/test_gpu_matern52grad.py except in two cases at d = 4 with one lengthscale: there it is drawn near 0.3, and the RBF's
# lighter tail leaves 48 % (product, 1024 x 256) and 46 % (derivative, 256 x 31) of the pair covariances inside (0.05, 0.95), below the half that
# ``_mixed`` asserts.  These two seeds are offset (same distributions; 75 % and 66 % then); every other case has at least 51 % as it stands.
RESEED = {("kv", 4, False, 3): 1000, ("grad", 4, False, 3): 10000}


def _kv_t(d):
    return sorted({1, 2, WIDEST_T[d], WIDEST_T[d] + 1, 11})


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


def _cloud(gen, n, d, offset=0.0):
    return _f32(torch.rand(n, d, generator=gen, dtype=torch.float64) + offset)


def _ls(gen, d, ard):
    ls = _f32(0.3 + 0.1 * torch.rand(d if ard else 1, generator=gen, dtype=torch.float64))
    assert ls.unique().numel() == ls.numel()                      # every lengthscale differs under ARD
    return ls


def _mixed(x1, x2, ls):
    """Share of the pair covariances k in (0.05, 0.95); a single pair must itself lie inside.  Depends on x and l only."""
    k = R.pair_covariances(x1, x2, ls)
    frac = float(((k > 0.05) & (k < 0.95)).double().mean())
    if k.numel() == 1:
        assert frac == 1.0, float(k)
    else:
        assert frac >= 0.5, frac
    return frac


def _prep(B, x, ls, shift, dev):
    return B.prep_points("rbf", x.float().to(dev), ls.float(), shift.float().to(dev))


def _kv_err(out, K, V):
    """Per column, relative to the column maximum of |K| |V|."""
    ref = K @ V.double()
    return float(((out.double().cpu() - ref).abs().max(0).values / (K.abs() @ V.double().abs()).max(0).values).max())


def _kv_check(B, x1, x2, ls, dev, what):
    d = x1.shape[1]
    c = 2 * d + 1
    same = x2 is None
    x2 = x1 if same else x2
    _mixed(x1, x2, ls)
    K = R.dense(x1, x2, ls)
    gen = torch.Generator().manual_seed(x1.shape[0] + 7 * x2.shape[0])
    V = torch.randn(x2.shape[0] * c, 11, generator=gen, dtype=torch.float64).float()
    shift = x1.mean(0)
    p1 = _prep(B, x1, ls, shift, dev)
    p2 = p1 if same else _prep(B, x2, ls, shift, dev)
    inv_ls = B.rbfgrad_inv_ls(ls.float(), d, dev)
    for t in _kv_t(d):
        out = B.from_probe_major(B.rbfgrad_kv(p1, p2, inv_ls, B.to_probe_major(V[:, :t].to(dev)), order=2), x1.shape[0] * c)
        err = _kv_err(out, K, V[:, :t])
        print("kv", what, tuple(x1.shape), tuple(x2.shape), "t", t, err)
        assert err < 2e-5, (what, x1.shape, x2.shape, t, err)


@pytest.mark.parametrize("ard", [False, True], ids=["single", "ard"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_kv_matches_restatement(d, ard, dev):
    from gpytorch_amd import backend as B

    for i, (n, m) in enumerate(KV_SIZES):
        gen = torch.Generator().manual_seed(100 * d + 10 * ard + i + RESEED.get(("kv", d, ard, i), 0))
        x1 = _cloud(gen, n, d)
        if n == 1:                                                # one point against another one a lengthscale away, not against itself
            x2 = _f32(x1 + 0.3)
        else:
            x2 = None if m == 0 else _cloud(gen, m, d)
        _kv_check(B, x1, x2, _ls(gen, d, ard), dev, f"d={d} ard={ard}")


def test_kv_with_all_coordinates_offset_by_1000(dev):
    """The prepared points are centred (the family's shift): a cloud around 1000 keeps the bound."""
    from gpytorch_amd import backend as B

    gen = torch.Generator().manual_seed(5)
    x1, x2 = _cloud(gen, 300, 3, 1000.0), _cloud(gen, 270, 3, 1000.0)
    _kv_check(B, x1, x2, _ls(gen, 3, True), dev, "offset 1000")


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_dense_rows_diagonal_and_operator_algebra(d, dev):
    import gpytorch_amd as g
    from gpytorch_amd.derivative import RBFGradGradFusedAddedDiagLinearOperator, RBFGradGradFusedLinearOperator
    from gpytorch_amd.operators import DenseLinearOperator, DiagLinearOperator

    c = 2 * d + 1
    n, m = 130, 47
    gen = torch.Generator().manual_seed(40 + d)
    x, x2 = _cloud(gen, n, d), _cloud(gen, m, d)
    ls = _ls(gen, d, True)
    _mixed(x, x2, ls)
    kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad(ard_num_dims=d)).to(dev)
    kern.base_kernel.lengthscale, kern.outputscale = ls.float().reshape(1, d), 1.7
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    plain = kern.base_kernel(xd)
    assert isinstance(plain, RBFGradGradFusedLinearOperator) and plain.outputscale is None
    op, rect = kern(xd), kern(xd, x2d)
    assert isinstance(op, RBFGradGradFusedLinearOperator) and op.shape == (n * c, n * c) and rect.shape == (n * c, m * c)
    Kref, Krect = 1.7 * R.dense(x, x, ls), 1.7 * R.dense(x, x2, ls)
    with torch.no_grad():
        assert rel_err(op.to_dense(), Kref) < 1e-5 and rel_err(rect.to_dense(), Krect) < 1e-5
        assert rel_err(op.diagonal(), Kref.diagonal()) < 1e-5
        assert rel_err(kern(xd, diag=True), Kref.diagonal()) < 1e-5
        with pytest.raises(RuntimeError, match="diag=True only works when x1 == x2"):
            kern(xd[:m], x2d, diag=True)
        # rows: what the pivoted-Cholesky preconditioner reads (k from the family's row kernel times the Hermite block)
        for p in (0, 1, d + 1, c, n * c - 1, (n // 2) * c + d):
            assert rel_err(op._row(torch.tensor([p], device=dev)), Kref[p]) < 1e-5, p
        # slices aligned to whole points stay matrix-free; anything else is dense
        sub = op[3 * c : 50 * c, 10 * c : 40 * c]
        assert isinstance(sub, RBFGradGradFusedLinearOperator) and sub.shape == (47 * c, 30 * c)
        assert rel_err(sub.to_dense(), Kref[3 * c : 50 * c, 10 * c : 40 * c]) < 1e-5
        assert isinstance(op[..., 3 * c :, : 3 * c], RBFGradGradFusedLinearOperator)
        cut = op[1 : 2 * c, :]
        assert isinstance(cut, DenseLinearOperator) and rel_err(cut.to_dense(), Kref[1 : 2 * c]) < 1e-5
        # products: the operator, its transpose, a slice, + diag
        V = torch.randn(n * c, 5, generator=gen, dtype=torch.float64).float()
        assert _kv_err(rect.mT @ V.to(dev), Krect.t(), V) < 2e-5
        assert _kv_err(op @ V.to(dev), Kref, V) < 2e-5
        assert _kv_err(sub @ V[: 30 * c].to(dev), Kref[3 * c : 50 * c, 10 * c : 40 * c], V[: 30 * c]) < 2e-5
        noise = _f32(0.05 + 0.1 * torch.rand(n * c, generator=gen, dtype=torch.float64))
        added = op + DiagLinearOperator(noise.float().to(dev))
        assert isinstance(added, RBFGradGradFusedAddedDiagLinearOperator)
        Kh = Kref + torch.diag(noise)
        assert rel_err(added.to_dense(), Kh) < 1e-5 and rel_err(added.diagonal(), Kh.diagonal()) < 1e-5
        assert _kv_err(added @ V.to(dev), Kh, V) < 2e-5
        twice = op.mul(2.0)
        assert isinstance(twice, RBFGradGradFusedLinearOperator) and _kv_err(twice @ V.to(dev), 2.0 * Kref, V) < 2e-5
        assert isinstance(op.detach(), RBFGradGradFusedLinearOperator)


def test_product_and_derivative_sums_are_bitwise_reproducible(dev):
    """No atomics anywhere: two calls return the same bits (several row blocks, several split-j slabs, column groups)."""
    from gpytorch_amd import backend as B

    d, n, m, t = 3, 1300, 1500, 6
    c = 2 * d + 1
    gen = torch.Generator().manual_seed(77)
    x1, x2 = _cloud(gen, n, d), _cloud(gen, m, d)
    ls = _ls(gen, d, True)
    shift = x1.mean(0)
    p1, p2 = _prep(B, x1, ls, shift, dev), _prep(B, x2, ls, shift, dev)
    inv_ls = B.rbfgrad_inv_ls(ls.float(), d, dev)
    Vt = B.to_probe_major(torch.randn(m * c, t, generator=gen).to(dev))
    Lt = B.to_probe_major(torch.randn(n * c, t, generator=gen).to(dev))
    a, b = B.rbfgrad_kv(p1, p2, inv_ls, Vt, order=2), B.rbfgrad_kv(p1, p2, inv_ls, Vt, order=2)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    s1, s2 = B.rbfgrad_kv_grad(p1, p2, inv_ls, Lt, Vt, order=2), B.rbfgrad_kv_grad(p1, p2, inv_ls, Lt, Vt, order=2)
    assert torch.equal(s1, s2) and s1.shape == (1 + d,) and bool(torch.isfinite(s1).all())


@pytest.mark.parametrize("ard", [False, True], ids=["single", "ard"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_bilinear_derivative_matches_autograd(d, ard, dev):
    """Lengthscale and outputscale gradients of sum_c l_c^T (outputscale K) r_c from the fused derivative kernel + ``functions.rbfgrad_hyper_grads``
    against float64 autograd of the restatement; one more case goes through the operator's own autograd (``op @ V``)."""
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import rbfgrad_hyper_grads

    c = 2 * d + 1
    for i, (n, m, coincide) in enumerate([(3, 3, True), (255, 257, False), (257, 257, True), (256, 31, False)]):
        gen = torch.Generator().manual_seed(1000 * d + 100 * ard + i + RESEED.get(("grad", d, ard, i), 0))
        x1 = _cloud(gen, n, d)
        x2 = x1 if coincide else _cloud(gen, m, d)
        ls64 = _ls(gen, d, ard).requires_grad_(True)
        os64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
        Lm = torch.randn(n * c, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(x2.shape[0] * c, 9, generator=gen, dtype=torch.float64).float()
        if n > 3:
            _mixed(x1, x2, ls64.detach())
        val = (Lm.double() * ((os64 * R.dense(x1, x2, ls64)) @ Rm.double())).sum()
        g_ls, g_os = torch.autograd.grad(val, [ls64, os64])
        shift = x1.mean(0)
        p1 = _prep(B, x1, ls64.detach(), shift, dev)
        p2 = p1 if coincide else _prep(B, x2, ls64.detach(), shift, dev)
        lsd, osd = ls64.detach().float().to(dev).reshape(1, -1), torch.tensor([1.3], device=dev)
        sums = B.rbfgrad_kv_grad(p1, p2, B.rbfgrad_inv_ls(lsd, d, dev), B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev)), order=2)
        assert bool(torch.isfinite(sums).all()), (n, m, d, ard, coincide, sums)
        d_ls, d_os = rbfgrad_hyper_grads(sums, lsd, osd)
        e_ls = float((d_ls.double().cpu().reshape(-1) - g_ls).abs().max() / g_ls.abs().max())
        e_os = abs(float(d_os) - float(g_os)) / abs(float(g_os))
        print("grad", (n, m, d), "ard" if ard else "single", "coincident" if coincide else "", e_ls, e_os)
        assert e_ls < 2e-3 and e_os < 2e-3, (n, m, d, ard, coincide, e_ls, e_os)
    # through the operator: raw parameters of ScaleKernel(RBFKernelGradGrad)
    kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad(ard_num_dims=d if ard else None)).to(dev)
    kern.base_kernel.lengthscale, kern.outputscale = ls64.detach().float().reshape(1, -1), 1.3
    o = kern(x1.float().to(dev), x2.float().to(dev))
    ((Lm.to(dev) * (o @ Rm.to(dev))).sum()).backward()
    sig = lambda raw: torch.sigmoid(raw.detach().double().cpu())  # noqa: E731   (d softplus / d raw)
    got_ls = kern.base_kernel.raw_lengthscale.grad.double().cpu() / sig(kern.base_kernel.raw_lengthscale)
    got_os = kern.raw_outputscale.grad.double().cpu() / sig(kern.raw_outputscale)
    assert float((got_ls.reshape(-1) - g_ls).abs().max() / g_ls.abs().max()) < 2e-3
    assert abs(float(got_os) - float(g_os)) / abs(float(g_os)) < 2e-3


# ---- the model: d = 2 data with analytic first and second derivatives; 5 tasks
HYP = dict(ls=0.4, os=1.3, tn=(0.05, 0.3, 0.3, 5.0, 5.0), noise=0.02, c=0.2)
E0 = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)


def _data(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    X = _f32(torch.rand(n, 2, generator=gen, dtype=torch.float64))
    a, b = 2 * math.pi * X[:, 0], math.pi * X[:, 1]
    F = torch.stack([a.sin() * b.cos(), 2 * math.pi * a.cos() * b.cos(), -math.pi * a.sin() * b.sin(),
                     -4 * math.pi ** 2 * a.sin() * b.cos(), -math.pi ** 2 * a.sin() * b.cos()], -1)
    sd = torch.tensor([0.2, 0.5, 0.5, 2.0, 2.0], dtype=torch.float64)
    return X, _f32(F + sd * torch.randn(n, 5, generator=gen, dtype=torch.float64))


def _model(g, X, Y, dev, dtype=torch.float32):
    class GPWithSecondDerivatives(g.models.ExactGP):
        def __init__(self, x, y, lik):
            super().__init__(x, y, lik)
            self.mean_module = g.means.ConstantMeanGradGrad()
            self.covar_module = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad())

        def forward(self, x):
            return g.distributions.MultitaskMultivariateNormal(self.mean_module(x), self.covar_module(x))

    lik = g.likelihoods.MultitaskGaussianLikelihood(num_tasks=5).to(dev).to(dtype)
    m = GPWithSecondDerivatives(X.to(dtype).to(dev), Y.to(dtype).to(dev), lik).to(dev).to(dtype)
    m.covar_module.base_kernel.lengthscale, m.covar_module.outputscale = HYP["ls"], HYP["os"]
    lik.task_noises, lik.noise = torch.tensor(HYP["tn"], dtype=dtype), HYP["noise"]
    with torch.no_grad():
        m.mean_module.constant.fill_(HYP["c"])
    return m, lik


def _khat(X, p):
    """Dense float64 K_hat and the flat prior mean for p = [lengthscale, outputscale, task noises [5], noise, constant]."""
    n = X.shape[0]
    Kh = p[1] * R.dense(X, X, p[0].reshape(1)) + torch.diag((p[2] + p[3]).repeat(n))
    return Kh, (p[4] * E0).repeat(n)


def _float32_dense_deviation(Kh, r, ref):
    """|MLL by float32 dense torch Cholesky on the host - float64 MLL| / max(1, |MLL|): what float32 alone costs at these inputs."""
    L = torch.linalg.cholesky(Kh.detach().float())
    rf = r.detach().float()
    quad = (rf * torch.cholesky_solve(rf.unsqueeze(-1), L).squeeze(-1)).sum()
    val = -0.5 * (quad + 2.0 * L.diagonal().log().sum() + rf.numel() * math.log(2.0 * math.pi)) / rf.numel()
    return abs(float(val) - float(ref.detach())) / max(1.0, abs(float(ref.detach())))


@pytest.mark.parametrize("branch", ["cholesky", "bbmm"])
def test_gp_mll_cholesky_and_bbmm(branch, dev):
    """ScaleKernel(RBFKernelGradGrad) + ConstantMeanGradGrad + MultitaskGaussianLikelihood(5): the marginal log likelihood and ALL hyper-gradients
    (lengthscale, outputscale, five task noises, global noise, mean constant) against dense float64 autograd: the Cholesky branch at n = 40, BBMM
    forced at n = 200 (``max_cholesky_size(0)``, the row-built preconditioner on, probes fixed by the seed and drawn from N(0, P), as in
    tests/test_gpu_matern52grad.py).  K_hat has 1000 rows and a condition number near 2e5 (second derivatives), so a solve takes about a hundred
    iterations on every probe column: 60 probes, not that test's 300, keep the case at a few seconds; the estimators' errors grow by
    sqrt(5) and the tolerances stay."""
    import gpytorch_amd as g
    from gpytorch_amd.derivative import RBFGradGradFusedLinearOperator

    n = 40 if branch == "cholesky" else 200
    tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
    X, Y = _data(n)
    p = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (HYP["ls"], HYP["os"], HYP["tn"], HYP["noise"], HYP["c"])]
    Kh, mean = _khat(X, p)
    ref = OG.dense_log_prob(Kh, Y.reshape(-1) - mean) / (5 * n)
    dev32 = _float32_dense_deviation(Kh, Y.reshape(-1) - mean, ref)
    print("mll", branch, "float32 dense Cholesky on the host deviates by", dev32, "cond(K_hat)", float(torch.linalg.cond(Kh.detach())))
    assert dev32 < tol_v / 4, (branch, dev32)                      # a condition on the inputs: K_hat is well conditioned for float32
    gref = torch.autograd.grad(ref, p)
    m, lik = _model(g, X, Y, dev)
    assert isinstance(m.covar_module(m.train_inputs[0]), RBFGradGradFusedLinearOperator)
    mll = g.ExactMarginalLogLikelihood(lik, m)
    m.train()
    lik.train()
    S = g.settings
    with warnings.catch_warnings(), S.max_cholesky_size(10_000 if branch == "cholesky" else 0), S.cg_tolerance(1e-5), S.num_trace_samples(60), \
            S.max_preconditioner_size(50), S.min_preconditioning_size(100), S.max_lanczos_quadrature_iterations(100):
        warnings.simplefilter("ignore")
        torch.manual_seed(0)                                       # fixes the probes, which are drawn from N(0, P) on the device
        val = mll(m(m.train_inputs[0]), m.train_targets)
        val.backward()
    assert math.isfinite(float(val.detach()))
    sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731   (d softplus / d raw at the value v)
    got = torch.cat([m.covar_module.base_kernel.raw_lengthscale.grad.reshape(-1), m.covar_module.raw_outputscale.grad.reshape(-1),
                     lik.raw_task_noises.grad.reshape(-1), lik.raw_noise.grad.reshape(-1), m.mean_module.constant.grad.reshape(-1)]).double().cpu()
    want = torch.cat([(gref[0] * sp(HYP["ls"])).reshape(-1), (gref[1] * sp(HYP["os"])).reshape(-1),
                      gref[2] * torch.tensor([sp(v - 1e-4) for v in HYP["tn"]], dtype=torch.float64), (gref[3] * sp(HYP["noise"] - 1e-4)).reshape(-1),
                      gref[4].reshape(-1)])
    e_v, e_g = abs(float(val.detach()) - float(ref.detach())) / max(1.0, abs(float(ref.detach()))), float((got - want).norm() / want.norm())
    print("mll", branch, e_v, e_g, got, want)
    assert e_v < tol_v, (branch, float(val), float(ref))
    assert e_g < tol_g, (branch, got, want)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_pred_var"])
def test_gp_posterior(fast, dev):
    """Posterior mean and variance of values, first and second derivatives at 50 test points against the dense float64 posterior: the train x test
    block is rectangular, which the reference's forward cannot form.  The posterior variance of a second derivative is what a prior variance of 157
    leaves after a reduction of about 150: the bound of 2e-3 relative to the largest posterior variance (10) asks the reduction K_s K_hat^-1 K_s^T
    for 1.3e-4, so the solves run at ``eval_cg_tolerance(1e-5)``, a factor ten below that (float32 dense Cholesky on the host: 1.3e-5)."""
    import gpytorch_amd as g

    n, ns = 200, 50
    X, Y = _data(n + ns)
    Xt, Yt, Xs = X[:n], Y[:n], X[n:]
    p = [torch.tensor(v, dtype=torch.float64) for v in (HYP["ls"], HYP["os"], HYP["tn"], HYP["noise"], HYP["c"])]
    Kh, mean = _khat(Xt, p)
    Lc = torch.linalg.cholesky(Kh)
    Ks = p[1] * R.dense(Xs, Xt, p[0].reshape(1))
    mu_ref = ((p[4] * E0).repeat(ns) + (Ks @ torch.cholesky_solve((Yt.reshape(-1) - mean).unsqueeze(-1), Lc)).squeeze(-1)).reshape(ns, 5)
    var_ref = (p[1] * R.diag(Xs, p[0].reshape(1)) + (p[2] + p[3]).repeat(ns)
               - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)).reshape(ns, 5)
    m, lik = _model(g, Xt, Yt, dev)
    m.eval()
    lik.eval()
    S = g.settings
    torch.manual_seed(1)
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-5), \
            S.max_root_decomposition_size(5 * n), S.min_preconditioning_size(100):
        warnings.simplefilter("ignore")
        pred = lik(m(Xs.float().to(dev)))
        mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
    assert mu.shape == (ns, 5) and var.shape == (ns, 5)
    e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
    print("posterior fast_pred_var", fast, e_mu, e_var)
    assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)


@pytest.mark.parametrize("chol", [10_000, 0], ids=["cholesky", "cg"])
def test_fantasy_model(chol, dev):
    """15 points of sin(2 pi x) with its first and second derivative: ``get_fantasy_model`` runs, and its mean agrees with a model conditioned on the
    concatenated data."""
    import gpytorch_amd as g

    gen = torch.Generator().manual_seed(2)
    w = 2 * math.pi

    def targets(x):
        return torch.hstack([torch.sin(w * x), w * torch.cos(w * x), -w * w * torch.sin(w * x)])

    tx = torch.linspace(0, 1, 15, dtype=torch.float64).reshape(-1, 1)
    nx = torch.rand(4, 1, generator=gen, dtype=torch.float64)
    ty, ny = targets(tx), targets(nx) + torch.tensor([0.1, 0.3, 2.0], dtype=torch.float64) * torch.randn(4, 3, generator=gen, dtype=torch.float64)
    xs = torch.rand(20, 1, generator=gen, dtype=torch.float64)

    def build(x, y):
        class GPWithSecondDerivatives(g.models.ExactGP):
            def __init__(self, x_, y_, lik_):
                super().__init__(x_, y_, lik_)
                self.mean_module = g.means.ConstantMeanGradGrad()
                self.covar_module = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad())

            def forward(self, x_):
                return g.distributions.MultitaskMultivariateNormal(self.mean_module(x_), self.covar_module(x_))

        lik = g.likelihoods.MultitaskGaussianLikelihood(num_tasks=3).to(dev)
        mod = GPWithSecondDerivatives(x.float().to(dev), y.float().to(dev), lik).to(dev)
        mod.covar_module.base_kernel.lengthscale = 0.3
        lik.task_noises, lik.noise = torch.tensor([0.05, 0.2, 5.0]), 0.01      # (3 / l^4 = 370: the second-derivative task carries the most noise)
        mod.eval()
        lik.eval()
        return mod

    S = g.settings
    with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(chol), S.eval_cg_tolerance(1e-5), S.cg_tolerance(1e-5):
        warnings.simplefilter("ignore")
        model = build(tx, ty)
        model(xs.float().to(dev))                                  # a posterior first: fills the caches
        fant = model.get_fantasy_model(nx.float().to(dev), ny.float().to(dev))
        assert fant.train_inputs[0].shape == (19, 1) and fant.train_targets.shape == (19, 3)
        mu_f = fant(xs.float().to(dev)).mean
        mu_c = build(torch.cat([tx, nx]), torch.cat([ty, ny]))(xs.float().to(dev)).mean
    assert mu_f.shape == (20, 3)
    e = rel_err(mu_f, mu_c)
    print("fantasy", chol, e)
    assert e < 2e-3, e


def test_is_matrix_free_at_size(dev):
    """n = 20 000, d = 3, eleven columns: N = 140 000, a dense float32 operator would be 78 GB.  The device memory ``op @ V`` adds at its peak stays
    below 1 GB and the result is finite; the 112 output rows of 16 sampled points are checked against the restatement."""
    import gpytorch_amd as g

    n, d, t = 20_000, 3, 11
    c = 2 * d + 1
    N = n * c
    gen = torch.Generator().manual_seed(5)
    x = _cloud(gen, n, d)
    ls = _ls(gen, d, True)
    V = torch.randn(N, t, generator=gen, dtype=torch.float64).float()
    kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad(ard_num_dims=d)).to(dev)
    kern.base_kernel.lengthscale, kern.outputscale = ls.float().reshape(1, d), 1.7
    xd, Vd = x.float().to(dev), V.to(dev)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = kern(xd) @ Vd
        torch.cuda.synchronize()
        added = torch.cuda.max_memory_allocated() - base
    print("peak bytes added", added, "dense K", 4 * N * N)
    assert added < 1 << 30, added
    assert out.shape == (N, t) and bool(torch.isfinite(out).all())
    pts = torch.randint(0, n, (16,), generator=gen)
    _mixed(x[pts], x, ls)
    Kr = 1.7 * R.dense(x[pts], x, ls)                     # [112, N]
    rows = (pts.unsqueeze(1) * c + torch.arange(c)).reshape(-1)
    err = _kv_err(out[rows.to(dev)], Kr, V)
    print("at size", err)
    assert err < 2e-5, err


def test_float64_model_takes_the_dense_branch(dev):
    """What the rule declines keeps the dense torch expression: a float64 model on the device equals the formula to 1e-10."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import DenseLinearOperator

    gen = torch.Generator().manual_seed(2)
    x, x2 = _cloud(gen, 60, 2), _cloud(gen, 35, 2)
    kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGradGrad(ard_num_dims=2)).to(dev).double()
    kern.base_kernel.lengthscale, kern.outputscale = torch.tensor([[0.35, 0.6]], dtype=torch.float64), 1.7
    out = kern(x.to(dev), x2.to(dev))
    assert isinstance(out, DenseLinearOperator) and out.dtype == torch.float64
    ref = 1.7 * R.dense(x, x2, torch.tensor([0.35, 0.6], dtype=torch.float64))
    assert rel_err(out.to_dense(), ref) < 1e-10
    assert rel_err(kern(x.to(dev), diag=True), 1.7 * R.diag(x, torch.tensor([0.35, 0.6], dtype=torch.float64))) < 1e-10
    # a float64 model end to end: the MLL by the dense branch
    X, Y = _data(30)
    m, lik = _model(g, X, Y, dev, torch.float64)
    m.train()
    lik.train()
    assert isinstance(m.covar_module(m.train_inputs[0]), DenseLinearOperator)
    p = [torch.tensor(v, dtype=torch.float64) for v in (HYP["ls"], HYP["os"], HYP["tn"], HYP["noise"], HYP["c"])]
    Kh, mean = _khat(X, p)
    want = float(OG.dense_log_prob(Kh, Y.reshape(-1) - mean) / (5 * 30))
    got = float(g.ExactMarginalLogLikelihood(lik, m)(m(m.train_inputs[0]), m.train_targets).detach())
    assert abs(got - want) < 1e-8 * max(1.0, abs(want)), (got, want)
    # d > 4 and inputs that ask for gradients stay dense in float32 too
    k5 = g.kernels.RBFKernelGradGrad().to(dev)
    assert isinstance(k5(torch.rand(9, 5, device=dev)), DenseLinearOperator)
    assert isinstance(g.kernels.RBFKernelGradGrad().to(dev)(torch.rand(9, 2, device=dev, requires_grad=True)), DenseLinearOperator)
