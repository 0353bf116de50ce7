"""GPU: the Gibbs covariance with a per-point lengthscale as ONE matrix-free operator (``GPAMD_GIBBS``; csrc/kv_directgibbs.hpp, csrc/kv_grad_gibbs.hpp,
``kernels.GibbsKernel``).

Oracle: tests/gibbs_ref.py, a float64 closed form written from the formula and pinned to the reference's own outputs (tests/test_gibbs_cpu.py).
Clouds are uniform on [0, 1]^d; the lengthscale of every point is uniform in [0.05 d, 0.3 d] for d = 1, 2, 3 and in [0.025 d, 0.3 d] = [0.15, 1.8]
for d = 6 (with the lower end 0.3 only 6 % of the entries fall below 0.2; chosen like the others, on the float64 oracle over three seeds: 11-13 % below
0.2, 12-13 % above 0.8, 23-27 % of the prefactors below 0.8).  Every case asserts its precondition on the float64 reference (``_mixed``): at least 5 %
of the (off-diagonal) entries below 0.2, at least 5 % above 0.8, at least 10 % of the pairs with a prefactor below 0.8.  Bounds -- those of
tests/test_gpu_additive.py / tests/test_gpu_product.py:
  * K V: per column, relative to the column's largest reference entry, 2e-5;
  * entries of K (dense, rows, diagonal) and rows of the pivoted-Cholesky factor, max-normalised: 1e-5;
  * gradients: 2e-3;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3, 5e-2 with fast_pred_var;
    fantasy model 4e-3."""
import copy
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from oracle import pivoted_cholesky as OPC
from tests.gibbs_ref import MLP, gibbs_diag, gibbs_grad_sums, gibbs_k, gibbs_K, prefactor
from tests.util import make_data, rel_err

pytestmark = pytest.mark.gpu

# (n, m, d, t); m = 0: the same cloud.  Both widths, fewer rows than one tile, ragged ends, every column-group boundary (1, 4, 5, 32, 33, 65, 70), two row
# tiles per wave (16 500 rows)
KV_SHAPES = [(300, 0, 1, 11), (257, 513, 2, 1), (65, 3000, 2, 4), (130, 1000, 3, 32), (1000, 129, 3, 33), (700, 700, 6, 65), (200, 600, 1, 70),
             (16_500, 300, 3, 33), (150, 260, 6, 5)]


def _f32(t):
    """Values the float32 kernels receive exactly, as float64."""
    return t.float().double()


def _cloud(gen, n, d):
    return _f32(torch.rand(n, d, generator=gen, dtype=torch.float64))


def _lrange(d):
    return (0.05 * d, 0.3 * d) if d <= 3 else (0.025 * d, 0.3 * d)


def _ls(gen, n, d):
    lo, hi = _lrange(d)
    return _f32(lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))


def _mixed(K, P, square=False):
    """K, P [n, m]: the reference covariances and prefactors of the pairs (``square``: one cloud, the diagonal does not count)."""
    if square:
        off = ~torch.eye(K.shape[0], dtype=torch.bool)
        K, P = K[off], P[off]
    lo, hi, pre = float((K < 0.2).double().mean()), float((K > 0.8).double().mean()), float((P < 0.8).double().mean())
    assert lo >= 0.05 and hi >= 0.05 and pre >= 0.10, (lo, hi, pre)


def _prep(B, X, l, shift, dev):
    z = torch.cat([X, l.reshape(-1, 1)], -1).float().to(dev)
    return B.prep_points("gibbs", z, torch.ones(1, 1, device=dev), torch.cat([shift, shift.new_zeros(1)]).float().to(dev))


def test_kv_matches_restatement(dev):
    from gpytorch_amd import backend as B

    for i, (n, m, d, t) in enumerate(KV_SHAPES):
        gen = torch.Generator().manual_seed(3000 + i)
        X1, l1 = _cloud(gen, n, d), _ls(gen, n, d)
        X2, l2 = (X1, l1) if m == 0 else (_cloud(gen, m, d), _ls(gen, m, d))
        V = torch.randn(X2.shape[0], t, generator=gen, dtype=torch.float64).float()
        K = gibbs_K(X1, l1, X2, l2)
        _mixed(K, prefactor(l1, l2), square=(m == 0))
        shift = X1.mean(0)
        p1 = _prep(B, X1, l1, shift, dev)
        p2 = p1 if m == 0 else _prep(B, X2, l2, shift, dev)
        assert p1.kind == "gibbs" and p1.dp == (4 if d <= 2 else 8) and p1.d == p1.dp
        assert B.kv_flags(p1, p2, t) == B.KV_SPLIT
        out = B.from_probe_major(B.kv(p1, p2, B.to_probe_major(V.to(dev))), n).double().cpu()
        ref = K @ V.double()
        err = float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())
        print("kv", (n, m, d, t), err)
        assert err < 2e-5, ((n, m, d, t), err)


def test_dense_rows_diag_pivoted_cholesky(dev):
    from gpytorch_amd import backend as B

    n, m = 300, 77
    for d in (1, 3, 6):
        gen = torch.Generator().manual_seed(50 + d)
        X1, X2, l1, l2 = _cloud(gen, n, d), _cloud(gen, m, d), _ls(gen, n, d), _ls(gen, m, d)
        shift = X1.mean(0)
        p1, p2 = _prep(B, X1, l1, shift, dev), _prep(B, X2, l2, shift, dev)
        assert p1.dp == (4 if d <= 2 else 8) and bool((p1.xp[:, 2 + d :] == 0).all())
        scale = torch.tensor([1.7], device=dev)
        _mixed(gibbs_K(X1, l1, X2, l2), prefactor(l1, l2))
        Kref = 1.7 * gibbs_K(X1, l1, X2, l2)
        e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
        rows = torch.tensor([0, n - 1, n // 2])
        e_r = rel_err(B.kernel_rows(p1, rows, p2, scale), Kref[rows])
        q1 = _prep(B, X1[:m], l1[:m], shift, dev)
        e_g = rel_err(B.kernel_diag(q1, p2, scale), 1.7 * gibbs_diag(X1[:m], l1[:m], X2, l2))
        assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n))               # exact unit diagonal
        # rows of the row-built pivoted-Cholesky factor: the device's pivots replayed in the float64 oracle (float32 ties make the sequence
        # rounding-dependent).  The row callback returns no pivot list; step k's pivot is where row k of the factor is largest: L[p_k, k] = sqrt(d_k[p_k])
        # and |L[i, k]| <= sqrt(d_k[i]) <= sqrt(d_k[p_k]) for every other i, p_k being the arg-max of the residual diagonal d_k
        rank = 10
        Kd = 1.7 * gibbs_K(X1, l1)
        Lt, piv, mm = B.pivoted_cholesky(p1, scale, rank, 1e-6)
        assert piv is None
        piv = Lt.argmax(dim=1).cpu()
        assert piv.unique().numel() == rank
        Lref, _, gaps = OPC.pivoted_cholesky(torch.full((n,), 1.7, dtype=torch.float64), lambda p: Kd[p], rank, 1e-6, forced_pivots=piv, return_gaps=True)
        assert mm == rank == Lref.shape[1] and max(gaps) < 1e-5, gaps
        e_p = rel_err(Lt.t(), Lref)
        print("entries", d, e_d, e_r, e_g, e_p)
        assert max(e_d, e_r, e_g, e_p) < 1e-5, (d, e_d, e_r, e_g, e_p)


def test_derivative_pass(dev):
    """``backend.kv_grad_gibbs`` against float64 autograd of sum W o K, W = L R^T with nine random columns: G0 and the per-point gradient vectors of both
    clouds, each measured as max_i |g_i - ref_i| / max_i |ref_i|; two runs are bitwise equal; a row whose lengthscale is 100 x its neighbours' stays
    finite and within the bound."""
    from gpytorch_amd import backend as B

    for n, m, d, coincide in [(210, 333, 1, False), (140, 90, 6, False), (150, 150, 3, True)]:
        gen = torch.Generator().manual_seed(7 + n)
        X1, l1 = _cloud(gen, n, d), _ls(gen, n, d)
        X2, l2 = (X1, l1) if coincide else (_cloud(gen, m, d), _ls(gen, m, d))
        _mixed(gibbs_K(X1, l1, X2, l2), prefactor(l1, l2), square=coincide)
        l1 = l1.clone()
        l1[n // 3] = _f32(100.0 * l1[n // 3])                                        # one row far outside the range of the others
        if coincide:
            l2 = l1
        Lm = torch.randn(n, 9, generator=gen, dtype=torch.float64).float()
        Rm = torch.randn(m, 9, generator=gen, dtype=torch.float64).float()
        g0, g1, g2 = gibbs_grad_sums(X1, l1, X2, l2, Lm.double() @ Rm.double().t())
        shift = X1.mean(0)
        p1 = _prep(B, X1, l1, shift, dev)
        p2 = p1 if coincide else _prep(B, X2, l2, shift, dev)
        lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
        G0, r1 = B.kv_grad_gibbs(p1, p2, lt, rt)
        H0, r2 = B.kv_grad_gibbs(p2, p1, rt, lt)
        assert r1.shape == (n,) and r2.shape == (m,) and bool(torch.isfinite(r1).all()) and bool(torch.isfinite(r2).all())
        G0b, r1b = B.kv_grad_gibbs(p1, p2, lt, rt)
        assert torch.equal(G0, G0b) and torch.equal(r1, r1b)                          # no atomics: the same bits
        e_0 = max(abs(float(G0) - float(g0)), abs(float(H0) - float(g0))) / abs(float(g0))
        e_1 = float((r1.double().cpu() - g1).abs().max() / g1.abs().max())
        e_2 = float((r2.double().cpu() - g2).abs().max() / g2.abs().max())
        e_wide = abs(float(r1[n // 3]) - float(g1[n // 3])) / float(g1.abs().max())
        print("grad", (n, m, d), "coincident" if coincide else "", e_0, e_1, e_2, e_wide)
        assert max(e_0, e_1, e_2, e_wide) < 2e-3, ((n, m, d), e_0, e_1, e_2, e_wide)


def _twin(fn):
    """The float64 CPU twin of a lengthscale_fn."""
    return copy.deepcopy(fn).to(device="cpu", dtype=torch.float64)


def _param_grads(fn):
    return torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in fn.parameters()])


@pytest.mark.parametrize("scaled", [False, True])
def test_kernel_api_builds_a_fused_gibbs_operator(scaled, dev):
    import gpytorch_amd as g
    from gpytorch_amd import kernels as KK
    from gpytorch_amd.operators import FusedKernelLinearOperator

    d, n, m = 1, 500, 333
    gen = torch.Generator().manual_seed(11)
    x, x2 = _cloud(gen, n, d), _cloud(gen, m, d)
    fn = MLP(d=d, seed=1, w2_scale=0.9, b2=-2.5)
    gib = g.kernels.GibbsKernel(fn)
    kern = (g.kernels.ScaleKernel(gib) if scaled else gib).to(dev)
    if scaled:
        kern.outputscale = 1.7
    osv = 1.7 if scaled else 1.0
    tw = _twin(fn)
    xd, x2d = x.float().to(dev), x2.float().to(dev)
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "gibbs" and op.shape == (n, n)
    assert op.x1.shape == (n, d + 1) and op.x1.requires_grad and not xd.requires_grad
    with torch.no_grad():
        lx, lx2 = tw(x), tw(x2)
        Kref = osv * KK.gibbs_dense(tw, x, x)
        assert rel_err(Kref, osv * gibbs_k(x, lx, x, lx)) < 1e-12
        assert rel_err(op.to_dense(), Kref) < 1e-5
        assert rel_err(kern(xd, x2d).to_dense(), osv * KK.gibbs_dense(tw, x, x2)) < 1e-5
        V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
        ref = Kref @ V.double()
        out = (op @ V.to(dev)).double().cpu()
        assert float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max()) < 2e-5
        # diag: the same input -> ones (times the outputscale), no launch; two different equally long inputs -> the elementwise values
        assert torch.allclose(kern(xd, diag=True).cpu(), torch.full((n,), osv))
        assert rel_err(kern(xd[:m], x2d, diag=True), osv * KK.gibbs_dense(tw, x[:m], x2, diag=True)) < 1e-5
        assert rel_err(op.diagonal(), torch.full((n,), osv)) < 1e-6
    # gradients of every parameter of the MLP (and the raw outputscale), through a product and through to_dense
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    o64 = torch.tensor(osv, dtype=torch.float64, requires_grad=True)
    for how in ("matmul", "dense"):
        tw.zero_grad()
        K64 = o64 * KK.gibbs_dense(tw, x, x)
        val64 = (U.double() * (K64 @ V.double())).sum() if how == "matmul" else (W.double() * K64).sum()
        (g_os,) = torch.autograd.grad(val64, [o64], retain_graph=True)
        val64.backward()
        want = _param_grads(tw)
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        got = _param_grads(fn)
        e = float((got - want).abs().max() / want.abs().max())
        print("api grad", scaled, how, e)
        assert e < 2e-3, (how, got, want)
        if scaled:
            got_os = float(kern.raw_outputscale.grad) / float(torch.sigmoid(kern.raw_outputscale.detach().double()))
            assert abs(got_os - float(g_os)) < 2e-3 * abs(float(g_os)), (how, got_os, float(g_os))


def test_outside_the_rule_takes_the_dense_branch(dev):
    """float64, d = 7, a batch and inputs that require grad are formed by ``gibbs_dense``: a DenseLinearOperator equal to the oracle to 1e-10."""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.operators import DenseLinearOperator

    gen = torch.Generator().manual_seed(3)

    def check(fn, x, tw=None):
        ker = g.kernels.GibbsKernel(fn).to(dev)
        op = ker(x.to(dev))
        assert isinstance(op, DenseLinearOperator)
        tw = _twin(fn) if tw is None else tw
        x64 = x.detach().double().cpu()
        ref = torch.stack([gibbs_k(xb, tw(xb), xb, tw(xb)) for xb in x64]) if x64.dim() == 3 else gibbs_k(x64, tw(x64), x64, tw(x64))
        return rel_err(operators.to_dense(op), ref.detach())

    x1 = torch.rand(60, 1, generator=gen, dtype=torch.float64)
    assert check(MLP(d=1, seed=2, dtype=torch.float64), x1) < 1e-10                                    # float64
    x7 = torch.rand(60, 7, generator=gen, dtype=torch.float64)
    assert check(MLP(d=7, seed=2, dtype=torch.float64), x7) < 1e-10                                    # d = 7 (float64 here so that 1e-10 is meaningful)
    ker7 = g.kernels.GibbsKernel(MLP(d=7, seed=2)).to(dev)
    assert isinstance(ker7(x7.float().to(dev)), DenseLinearOperator)                                    # ... and float32 at d = 7 is dense too
    xb = torch.rand(2, 40, 2, generator=gen, dtype=torch.float64)
    assert check(MLP(d=2, seed=2, dtype=torch.float64), xb) < 1e-10                                    # a batch
    kb = g.kernels.GibbsKernel(MLP(d=2, seed=2)).to(dev)
    assert isinstance(kb(xb.float().to(dev)), DenseLinearOperator)
    # inputs that require grad: float32 is dense (the native family has no input gradients); in float64 the values and the input gradient are the oracle's
    x32 = torch.rand(50, 2, generator=gen, dtype=torch.float64).float()
    fn = MLP(d=2, seed=2)
    assert isinstance(g.kernels.GibbsKernel(fn).to(dev)(x32.to(dev)), operators.FusedKernelLinearOperator)
    assert isinstance(g.kernels.GibbsKernel(fn).to(dev)(x32.to(dev).requires_grad_(True)), DenseLinearOperator)
    fn64 = MLP(d=2, seed=2, dtype=torch.float64)
    tw = _twin(fn64)
    xg = x32.double().to(dev).requires_grad_(True)
    op = g.kernels.GibbsKernel(fn64).to(dev)(xg)
    assert isinstance(op, DenseLinearOperator)
    x64 = x32.double().requires_grad_(True)
    ref = gibbs_k(x64, tw(x64), x64, tw(x64))
    assert rel_err(operators.to_dense(op), ref) < 1e-10
    Wg = torch.randn(50, 50, generator=gen, dtype=torch.float64)
    (Wg.to(dev) * operators.to_dense(op)).sum().backward()
    (Wg * ref).sum().backward()
    assert rel_err(xg.grad, x64.grad) < 1e-8


MODEL_OS, MODEL_NOISE = 1.3, 0.1


def _model_fn(dtype=torch.float32):
    return MLP(d=1, seed=1, dtype=dtype, w2_scale=0.9, b2=-2.5)     # l(x) in [0.08, 0.23] on [0, 1]


class Narrow(torch.nn.Module):
    """l(x) = 0.2 + 0.05 sigmoid(w (x - 1/2) + b) in [0.2, 0.25]: the nearly-constant regime in which the d >= 2 kernel is usable."""

    def __init__(self, d=2, seed=0, dtype=torch.float32):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(3.0 * torch.randn(d, 1, generator=gen, dtype=dtype))
        self.b = torch.nn.Parameter(torch.zeros(1, dtype=dtype))

    def forward(self, x):
        return 0.2 + 0.05 * torch.sigmoid((x - 0.5) @ self.w + self.b)


def _gp_class(g, make_fn):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(g.kernels.GibbsKernel(make_fn()))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _set_model(m, lik):
    m.covar_module.outputscale = MODEL_OS
    lik.noise = MODEL_NOISE


def _reference_mll(make_fn, X, y):
    """(value, gradient vector [lengthscale_fn parameters | outputscale | noise]) of the marginal log likelihood per point, dense float64 autograd; asserts
    the precondition: the smallest eigenvalue of K + sigma^2 I is at least sigma^2 / 2."""
    n = X.shape[0]
    tw = make_fn(torch.float64)
    os_, nz = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (MODEL_OS, MODEL_NOISE))
    l = tw(X)
    Khat = os_ * gibbs_k(X, l, X, l) + nz * torch.eye(n, dtype=torch.float64)
    assert float(torch.linalg.eigvalsh(Khat.detach()).min()) >= MODEL_NOISE / 2
    ref = OG.dense_log_prob(Khat, y) / n
    gref = torch.autograd.grad(ref, list(tw.parameters()) + [os_, nz])
    sp = lambda v: 1.0 - math.exp(-v)  # noqa: E731   (d softplus / d raw at the value v)
    want = torch.cat([t.reshape(-1) for t in gref[:-2]] + [gref[-2].reshape(1) * sp(MODEL_OS), gref[-1].reshape(1) * sp(MODEL_NOISE - 1e-4)])
    return ref.detach(), want


def _model_mll(g, M, X, y, dev, branch):
    from gpytorch_amd.operators import FusedKernelLinearOperator

    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
    _set_model(m, lik)
    op = m.covar_module(m.train_inputs[0])
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "gibbs"
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
    got = torch.cat([_param_grads(m.covar_module.base_kernel.lengthscale_fn), m.covar_module.raw_outputscale.grad.detach().double().cpu().reshape(1),
                     lik.noise_covar.raw_noise.grad.detach().double().cpu().reshape(-1).sum().reshape(1)])
    return float(val.detach()), got


def test_gp_mll_cholesky_and_bbmm_d1(dev):
    """ScaleKernel(GibbsKernel(MLP)) + Gaussian noise, d = 1, n = 600: the marginal log likelihood and the gradients of every MLP parameter, the
    outputscale and the noise, on the Cholesky branch and on the BBMM branch (``max_cholesky_size(0)``, deterministic probes), against dense float64
    autograd, with the settings and bounds of tests/test_gpu_additive.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g

    X, y = make_data(600, 1)
    X, y = _f32(X), _f32(y)
    ref, want = _reference_mll(_model_fn, X, y)
    M = _gp_class(g, _model_fn)
    for branch in ("cholesky", "bbmm"):
        val, got = _model_mll(g, M, X, y, dev, branch)
        tol_v, tol_g = (2e-4, 3e-3) if branch == "cholesky" else (5e-3, 0.15)
        e_v, e_g = abs(val - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("mll d=1", branch, e_v, e_g)
        assert e_v < tol_v, (branch, val, float(ref))
        assert e_g < tol_g, (branch, got, want)


def test_gp_mll_cholesky_d2_nearly_constant_lengthscale(dev):
    """d = 2, n = 400, l in [0.2, 0.25] -- the nearly-constant regime the class docstring names: Cholesky-branch value and gradients."""
    import gpytorch_amd as g

    make_fn = lambda dtype=torch.float32: Narrow(d=2, seed=0, dtype=dtype)  # noqa: E731
    X, y = make_data(400, 2)
    X, y = _f32(X), _f32(y)
    with torch.no_grad():
        l = make_fn(torch.float64)(X)
        assert 0.2 <= float(l.min()) and float(l.max()) <= 0.25 and float(l.max() - l.min()) > 0.02
    ref, want = _reference_mll(make_fn, X, y)
    val, got = _model_mll(g, _gp_class(g, make_fn), X, y, dev, "cholesky")
    e_v, e_g = abs(val - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
    print("mll d=2", e_v, e_g)
    assert e_v < 2e-4, (val, float(ref))
    assert e_g < 3e-3, (got, want)


def test_gp_posterior_fast_pred_var_and_fantasy(dev):
    """Posterior mean and variance of the d = 1 model against the dense float64 posterior, exact and with ``fast_pred_var`` (LOVE), then a fantasy model
    on 40 more observations against the dense posterior of the enlarged data set: settings and bounds of
    tests/test_gpu_additive.py::test_gp_posterior_fast_pred_var_and_fantasy."""
    import gpytorch_amd as g

    n, nf, ns = 600, 40, 200
    X, y = make_data(n + nf + ns, 1)
    X, y = _f32(X), _f32(y)
    Xt, yt, Xf, yf, Xs = X[:n], y[:n], X[n : n + nf], y[n : n + nf], X[n + nf :]
    tw = _model_fn(torch.float64)

    def cov(A, Bm):
        with torch.no_grad():
            return MODEL_OS * gibbs_k(A, tw(A), Bm, tw(Bm))

    def dense_posterior(Xa, ya):
        Khat = cov(Xa, Xa) + MODEL_NOISE * torch.eye(Xa.shape[0], dtype=torch.float64)
        assert float(torch.linalg.eigvalsh(Khat).min()) >= MODEL_NOISE / 2
        Lc = torch.linalg.cholesky(Khat)
        Ks = cov(Xs, Xa)
        mu = (Ks @ torch.cholesky_solve(ya.unsqueeze(-1), Lc)).squeeze(-1)
        return mu, MODEL_OS + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)

    mu_ref, var_ref = dense_posterior(Xt, yt)
    M = _gp_class(g, _model_fn)
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
