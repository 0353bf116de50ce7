"""GPU: the inverse-multiquadric Hamming kernel as ONE matrix-free operator over packed tokens (``KIND_HAMMING``; csrc/kv_directham.hpp,
csrc/kv_grad_ham.hpp, ``kernels.HammingIMQKernel``), modelled on tests/test_gpu_product_structure.py.

Oracle: tests/hamming_ref.py, float64 on TOKENS from the formula k = ((1 + alpha) / (alpha + c))^beta, pinned to the reference's own outputs
(tests/test_hamming_cpu.py).  Clouds are mutated copies of three parent sequences (every row redraws each position with its own probability in
0..0.5), so the distances of a case spread over 0..T instead of piling up at T (1 - 1/V) as for uniform tokens, where every off-diagonal value is the
same tiny number; the second cloud starts with copies of rows of the first, so c = 0 occurs off the diagonal.  Shapes are the smallest at which each
path begins: 1 / 127 / 129 / 300 rows (one lane, a ragged and a second 128-row block), 1 / 129 / 517 contracted points (a ragged 128-tile, more than
one j chunk), 1 / 4 / 5 / 32 / 33 / 34 / 65 columns (one column, the 32-column tile, its extra VALU column, a second launch group), T = 1 / 16 | 17 /
64 | 65 / 127 / 128 (the four prepared widths and their edges), V = 2 / 20 / 126 (the smallest, a protein alphabet, the largest byte).  Bounds -- those
of tests/test_gpu_product_structure.py for the same quantities:
  * K V: per column, relative to the column's largest reference entry, 2e-5;
  * entries of K (dense, rows, diagonal), max-normalised: 1e-5; c = 0 gives exactly 1;
  * the three derivative sums: 2e-3;
  * the model: marginal log likelihood 2e-4 / 3e-3 on the Cholesky branch, 5e-3 / 0.15 on the BBMM branch; posterior 2e-3, 5e-2 with fast_pred_var."""
import math
import warnings

import pytest
import torch

from oracle import exact_gp as OG
from tests.hamming_ref import hamming_counts, hamming_grad_sums, hamming_k, hamming_kt, one_hot
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def _parents(gen, t, v):
    return torch.randint(0, v, (3, t), generator=gen)


def _cloud(gen, n, t, v, parents, copy_of=None):
    """[n, T] tokens: a parent per row, every position redrawn with the row's own probability in 0..0.5; the first rows copies of ``copy_of``."""
    par = parents[torch.randint(0, parents.shape[0], (n,), generator=gen)]
    redraw = torch.rand(n, t, generator=gen) < 0.5 * torch.rand(n, 1, generator=gen)
    tok = torch.where(redraw, torch.randint(0, v, (n, t), generator=gen), par)
    if copy_of is not None:
        k = min(n, copy_of.shape[0], 40)
        tok[:k] = copy_of[:k]
    return tok


def _spread(c, t):
    """The distances of a case take several values, zero among them off the diagonal where the clouds share rows."""
    if c.numel() >= 100:
        assert c.unique().numel() >= min(t + 1, 5), c.unique()


def _prep(B, tok, v, alpha, beta, dev):
    return B.prep_points("hamming", one_hot(tok, v).to(dev), torch.ones(1, 1), None, (v, torch.tensor([alpha, beta])))


# (n, m or 0 for one cloud, T, V, columns, alpha, beta)
KV_SHAPES = [(1, 0, 1, 2, 1, 0.3, 0.5), (127, 0, 16, 20, 4, 1.0, 1.5), (129, 0, 17, 126, 5, 3.0, 3.0), (300, 0, 64, 20, 32, 0.7, 2.0),
             (300, 0, 65, 2, 33, 2.0, 0.5), (129, 0, 127, 20, 34, 0.5, 1.0), (300, 0, 128, 126, 65, 1.5, 2.5),
             (1, 1, 16, 20, 1, 0.9, 1.1), (127, 129, 64, 2, 33, 1.3, 0.8), (300, 517, 128, 20, 65, 0.4, 1.7), (129, 1, 17, 126, 5, 2.5, 3.0),
             (300, 517, 1, 2, 34, 0.6, 2.2), (1, 517, 65, 20, 4, 1.9, 0.6), (300, 129, 127, 126, 32, 3.0, 0.5)]


def test_shapes_cover_the_paths():
    cols = list(zip(*KV_SHAPES))
    assert set(cols[0]) == {1, 127, 129, 300} and set(cols[1]) == {0, 1, 129, 517} and set(cols[4]) == {1, 4, 5, 32, 33, 34, 65}
    assert set(cols[2]) == {1, 16, 17, 64, 65, 127, 128} and set(cols[3]) == {2, 20, 126}
    assert all(0.3 <= a <= 3.0 and 0.5 <= b <= 3.0 for a, b in zip(cols[5], cols[6]))


@pytest.mark.parametrize("case", KV_SHAPES, ids=lambda c: "n%d_m%d_T%d_V%d_t%d" % c[:5])
def test_kv_matches_float64(case, dev):
    """K~ V, square and rectangular, against a float64 dense product; two launches give identical bits."""
    from gpytorch_amd import backend as B

    n, m, t, v, cols, alpha, beta = case
    gen = torch.Generator().manual_seed(1000 + KV_SHAPES.index(case))
    par = _parents(gen, t, v)
    tok1 = _cloud(gen, n, t, v, par)
    tok2 = None if m == 0 else _cloud(gen, m, t, v, par, copy_of=tok1)
    V = torch.randn(n if m == 0 else m, cols, generator=gen, dtype=torch.float64).float()
    c = hamming_counts(tok1, tok2)
    _spread(c, t)
    p1 = _prep(B, tok1, v, alpha, beta, dev)
    p2 = p1 if tok2 is None else _prep(B, tok2, v, alpha, beta, dev)
    assert p1.dp == B.hamming_width(t) == p1.d and p1.xp.dtype == torch.float32 and B.kv_flags(p1, p2, cols) == B.KV_SPLIT
    vt = B.to_probe_major(V.to(dev))
    out_t = B.kv(p1, p2, vt)
    assert torch.equal(out_t[:, :n], B.kv(p1, p2, vt)[:, :n])                      # fixed summation order: bitwise run to run (beyond n: padding)
    out = B.from_probe_major(out_t, n).double().cpu()
    ref = hamming_kt(c, alpha, beta) @ V.double()
    err = float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max())
    print("kv", case, err)
    assert err < 2e-5, (case, err)


ENTRY_SHAPES = [(300, 129, 1, 2, 0.3, 3.0), (129, 517, 16, 20, 1.0, 0.5), (127, 129, 17, 126, 3.0, 1.5), (300, 129, 64, 20, 0.7, 2.0),
                (129, 300, 65, 2, 2.0, 1.0), (300, 127, 127, 20, 0.5, 2.5), (127, 517, 128, 126, 1.5, 3.0)]


@pytest.mark.parametrize("case", ENTRY_SHAPES, ids=lambda c: "n%d_m%d_T%d_V%d" % c[:4])
def test_dense_rows_diag_and_exact_ones(case, dev):
    """Entries of K (dense, rows, diagonal of pairs) against float64, max-normalised, 1e-5; where both clouds share rows c = 0 gives EXACTLY 1."""
    from gpytorch_amd import backend as B

    n, m, t, v, alpha, beta = case
    gen = torch.Generator().manual_seed(50 + ENTRY_SHAPES.index(case))
    par = _parents(gen, t, v)
    tok1 = _cloud(gen, n, t, v, par)
    tok2 = _cloud(gen, m, t, v, par, copy_of=tok1)
    c = hamming_counts(tok1, tok2)
    _spread(c, t)
    p1, p2 = _prep(B, tok1, v, alpha, beta, dev), _prep(B, tok2, v, alpha, beta, dev)
    by = p1.xp.view(torch.int8)
    assert bool(torch.isfinite(p1.xp).all()) and int(by.min()) >= 1 and torch.equal(by[:, :t].cpu(), (tok1 + 1).to(torch.int8)) and bool((by[:, t:] == 1).all())
    scale = torch.tensor([1.7], device=dev)
    Kref = 1.7 * hamming_kt(c, alpha, beta)
    e_d = rel_err(B.kernel_dense(p1, p2, scale), Kref)
    rows = torch.tensor([0, n - 1, n // 2])
    e_r = rel_err(B.kernel_rows(p1, rows.to(dev), p2, scale), Kref[rows])
    k = min(n, m)
    q1, q2 = _prep(B, tok1[:k], v, alpha, beta, dev), _prep(B, tok2[:k], v, alpha, beta, dev)
    e_g = rel_err(B.kernel_diag(q1, q2, scale), Kref[:k, :k].diagonal())
    print("entries", case, e_d, e_r, e_g)
    assert max(e_d, e_r, e_g) < 1e-5, (case, e_d, e_r, e_g)
    K = B.kernel_dense(p1, p2).cpu()
    zero = c == 0
    assert int(zero.sum()) >= min(n, m, 40) and bool((K[zero] == 1.0).all()) and bool((K[~zero] < 1.0).all())
    assert torch.equal(B.kernel_diag(q1, q2).cpu()[: min(k, 40)], torch.ones(min(k, 40)))           # the copied rows, pair by pair
    assert torch.equal(B.kernel_diag(p1, p1).cpu(), torch.ones(n)) and torch.equal(B.kernel_dense(p1, p1).diagonal().cpu(), torch.ones(n))


GRAD_SHAPES = [(210, 333, 17, 20, 9, 0.7, 1.5), (129, 129, 128, 126, 5, 2.0, 0.5), (300, 517, 1, 2, 34, 0.3, 3.0), (127, 1, 64, 20, 1, 1.2, 2.0),
               (150, 0, 65, 2, 9, 3.0, 1.0), (300, 129, 16, 126, 33, 0.5, 2.5)]


@pytest.mark.parametrize("case", GRAD_SHAPES, ids=lambda c: "n%d_m%d_T%d_V%d_t%d" % c[:5])
def test_derivative_sums(case, dev):
    """The three sums of csrc/kv_grad_ham.hpp against float64 closed forms with W = L R^T, each relative to its own reference value, 2e-3; two calls
    give identical bits; ``functions.hyper_grads`` turns them into the gradients of the slots; input gradients are refused."""
    from gpytorch_amd import backend as B
    from gpytorch_amd.functions import hyper_grads

    n, m, t, v, cols, alpha, beta = case
    gen = torch.Generator().manual_seed(7 + GRAD_SHAPES.index(case))
    par = _parents(gen, t, v)
    tok1 = _cloud(gen, n, t, v, par)
    tok2 = tok1 if m == 0 else _cloud(gen, m, t, v, par, copy_of=tok1)
    m = n if m == 0 else m
    Lm = torch.randn(n, cols, generator=gen, dtype=torch.float64).float()
    Rm = torch.randn(m, cols, generator=gen, dtype=torch.float64).float()
    c = hamming_counts(tok1, tok2)
    _spread(c, t)
    want = hamming_grad_sums(c, alpha, beta, Lm.double() @ Rm.double().t())
    p1 = _prep(B, tok1, v, alpha, beta, dev)
    p2 = p1 if tok2 is tok1 else _prep(B, tok2, v, alpha, beta, dev)
    lt, rt = B.to_probe_major(Lm.to(dev)), B.to_probe_major(Rm.to(dev))
    s1, s2 = B.kv_grad_hamming(p1, p2, lt, rt), B.kv_grad_hamming(p1, p2, lt, rt)
    assert s1.shape == (3,) and s1.dtype == torch.float32 and torch.equal(s1, s2)      # fixed-order float64 accumulation, no atomics
    errs = ((s1.double().cpu() - want).abs() / want.abs()).tolist()
    print("grad sums", case, errs, want.tolist())
    assert max(errs) < 2e-3, (case, errs)
    ones, osd = torch.ones(1, 1, device=dev), torch.tensor([1.3], device=dev)
    theta = torch.tensor([alpha, beta], device=dev)
    d_ls, d_os, d_th = hyper_grads(p1, p2, ones, osd, lt, rt, kparam=theta)
    assert torch.equal(d_ls, torch.zeros(1, 1, device=dev)) and abs(float(d_os) - float(want[0])) < 2e-3 * abs(float(want[0]))
    ref_th = torch.stack([-1.3 * want[1] / alpha, 1.3 * want[2]])
    assert float(((d_th.double().cpu() - ref_th).abs() / ref_th.abs()).max()) < 2e-3
    with pytest.raises(RuntimeError, match="'hamming'"):
        hyper_grads(p1, p2, ones, osd, lt, rt, want_x1=True)


MODEL_T, MODEL_V, MODEL_ALPHA, MODEL_BETA, MODEL_OS, MODEL_NOISE = 65, 20, 1.2, 1.5, 1.3, 0.1


def _model_data(n, seed=0):
    """Sequences (mutated parents) and a fitness that depends on five positions, plus noise."""
    gen = torch.Generator().manual_seed(seed)
    tok = _cloud(gen, n, MODEL_T, MODEL_V, _parents(gen, MODEL_T, MODEL_V))
    w = torch.randn(5, MODEL_V, generator=gen, dtype=torch.float64)
    y = sum(w[i][tok[:, 7 * i + 3]] for i in range(5)) / math.sqrt(5.0) + 0.1 * torch.randn(n, generator=gen, dtype=torch.float64)
    return tok, y.float().double()


def _gp_class(g):
    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = g.kernels.ScaleKernel(g.kernels.HammingIMQKernel(vocab_size=MODEL_V))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    return M


def _set_model(m, lik):
    m.covar_module.base_kernel.alpha, m.covar_module.base_kernel.beta = MODEL_ALPHA, MODEL_BETA
    m.covar_module.outputscale = MODEL_OS
    lik.noise = MODEL_NOISE


def _sp(v):
    return 1.0 - math.exp(-v)   # d softplus / d raw at the value v


def test_gp_mll_cholesky_and_bbmm(dev):
    """ScaleKernel(HammingIMQKernel) + Gaussian noise, n = 400, T = 65 (the widest rows), V = 20: the marginal log likelihood and the gradients of
    alpha, beta, outputscale and noise on the Cholesky branch and on the BBMM branch (``max_cholesky_size(0)``: mBCG + SLQ with the row-built
    pivoted-Cholesky preconditioner, the same deterministic probes) against dense float64 autograd, with the settings and bounds of
    tests/test_gpu_product_structure.py::test_gp_mll_cholesky_and_bbmm."""
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    n = 400
    tok, y = _model_data(n)
    c = hamming_counts(tok)
    _spread(c, MODEL_T)
    al, be, os_, nz = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (MODEL_ALPHA, MODEL_BETA, MODEL_OS, MODEL_NOISE))
    ref = OG.dense_log_prob(os_ * hamming_k(c, al, be) + nz * torch.eye(n, dtype=torch.float64), y) / n
    gref = torch.autograd.grad(ref, [al, be, os_, nz])
    want = torch.tensor([float(gref[0]) * _sp(MODEL_ALPHA), float(gref[1]) * _sp(MODEL_BETA), float(gref[2]) * _sp(MODEL_OS),
                         float(gref[3]) * _sp(MODEL_NOISE - 1e-4)], dtype=torch.float64)
    M = _gp_class(g)
    X = one_hot(tok, MODEL_V)
    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.to(dev), y.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        op = m.covar_module(m.train_inputs[0])
        assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "hamming"
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
        hk = m.covar_module.base_kernel
        got = torch.tensor([float(hk.raw_alpha.grad), float(hk.raw_beta.grad), float(m.covar_module.raw_outputscale.grad),
                            float(lik.noise_covar.raw_noise.grad.sum())], dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        e_each = ((got - want).abs() / want.abs()).tolist()
        print("mll", branch, e_v, e_g, e_each, got, want)
        assert e_v < tol_v, (branch, float(val), float(ref))
        assert e_g < tol_g, (branch, got, want)


def test_gp_posterior(dev):
    """Posterior mean and variance of the same model (n = 400) against the dense float64 posterior, exact and with ``fast_pred_var`` (LOVE): 2e-3, and
    5e-2 for the LOVE variances."""
    import gpytorch_amd as g

    n, ns = 400, 100
    tok, y = _model_data(n + ns, seed=1)
    tt, yt, ts = tok[:n], y[:n], tok[n:]
    k0 = ((1 + MODEL_ALPHA) / MODEL_ALPHA) ** MODEL_BETA
    Lc = torch.linalg.cholesky(MODEL_OS * hamming_k(hamming_counts(tt), MODEL_ALPHA, MODEL_BETA) + MODEL_NOISE * torch.eye(n, dtype=torch.float64))
    Ks = MODEL_OS * hamming_k(hamming_counts(ts, tt), MODEL_ALPHA, MODEL_BETA)
    mu_ref = (Ks @ torch.cholesky_solve(yt.unsqueeze(-1), Lc)).squeeze(-1)
    var_ref = MODEL_OS * k0 + MODEL_NOISE - torch.linalg.solve_triangular(Lc, Ks.t(), upper=False).pow(2).sum(0)
    M = _gp_class(g)
    S = g.settings
    for fast in (True, False):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(one_hot(tt, MODEL_V).to(dev), yt.float().to(dev), lik).to(dev)
        _set_model(m, lik)
        m.eval()
        lik.eval()
        torch.manual_seed(1)
        with torch.no_grad(), warnings.catch_warnings(), S.max_cholesky_size(0), S.fast_pred_var(fast), S.eval_cg_tolerance(1e-4 if fast else 1e-6), \
                S.max_root_decomposition_size(400):
            warnings.simplefilter("ignore")
            pred = lik(m(one_hot(ts, MODEL_V).to(dev)))
            mu, var = pred.mean.double().cpu(), pred.variance.double().cpu()
        e_mu, e_var = rel_err(mu, mu_ref), rel_err(var, var_ref)
        print("posterior fast_pred_var", fast, e_mu, e_var)
        assert e_mu < 2e-3 and e_var < (5e-2 if fast else 2e-3), (fast, e_mu, e_var)


def test_kernel_api_and_routing(dev):
    """On the device: one-hot float32 inputs give ONE fused operator of kind "hamming" whose dense form, products and parameter gradients match
    float64; inputs that are not one-hot, T = 129 and float64 give a ``DenseLinearOperator`` with the dense branch's values."""
    import gpytorch_amd as g
    from gpytorch_amd import operators
    from gpytorch_amd.operators import DenseLinearOperator, FusedKernelLinearOperator

    t, v, n, m = 33, 20, 300, 129
    gen = torch.Generator().manual_seed(11)
    par = _parents(gen, t, v)
    tok, tok2 = _cloud(gen, n, t, v, par), _cloud(gen, m, t, v, par)
    kern = g.kernels.ScaleKernel(g.kernels.HammingIMQKernel(vocab_size=v)).to(dev)
    hk = kern.base_kernel
    hk.alpha, hk.beta, kern.outputscale = 0.8, 1.7, 1.2
    xd, x2d = one_hot(tok, v).to(dev), one_hot(tok2, v).to(dev)
    op = kern(xd)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "hamming" and op.shape == (n, n)
    Kref = 1.2 * hamming_k(hamming_counts(tok), 0.8, 1.7)
    assert rel_err(op.to_dense(), Kref) < 1e-5 and rel_err(kern(xd, x2d).to_dense(), 1.2 * hamming_k(hamming_counts(tok, tok2), 0.8, 1.7)) < 1e-5
    V = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    ref = Kref @ V.double()
    out = (op @ V.to(dev)).detach().double().cpu()
    assert float(((out - ref).abs().max(0).values / ref.abs().max(0).values).max()) < 2e-5
    k0 = 1.2 * (1.8 / 0.8) ** 1.7
    assert rel_err(kern(xd, diag=True), torch.full((n,), k0)) < 1e-6 and rel_err(op.diagonal(), torch.full((n,), k0)) < 1e-6
    assert rel_err(kern(xd[:m], x2d, diag=True), 1.2 * hamming_k((tok[:m] != tok2).sum(-1).double(), 0.8, 1.7)) < 1e-5
    # gradients of raw alpha, raw beta and the raw outputscale through a product and through to_dense
    U = torch.randn(n, 11, generator=gen, dtype=torch.float64).float()
    W = torch.randn(n, n, generator=gen, dtype=torch.float64).float()
    a64, b64, o64 = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (0.8, 1.7, 1.2))
    K64 = o64 * hamming_k(hamming_counts(tok), a64, b64)
    gref = torch.autograd.grad((U.double() * (K64 @ V.double())).sum(), [a64, b64, o64], retain_graph=True)
    gref_d = torch.autograd.grad((W.double() * K64).sum(), [a64, b64, o64])
    for how, want in (("matmul", gref), ("dense", gref_d)):
        for p in kern.parameters():
            p.grad = None
        o = kern(xd)
        val = (U.to(dev) * (o @ V.to(dev))).sum() if how == "matmul" else (W.to(dev) * o.to_dense()).sum()
        val.backward()
        got = [float(hk.raw_alpha.grad) / _sp(0.8), float(hk.raw_beta.grad) / _sp(1.7), float(kern.raw_outputscale.grad) / _sp(1.2)]
        errs = [abs(a - float(b)) / abs(float(b)) for a, b in zip(got, want)]
        print("api grad", how, errs)
        assert max(errs) < 2e-3, (how, got, want)
    # declined calls: the dense branch's values
    soft = xd.clone()
    soft[0, :v] = 0.0
    soft[0, :2] = 0.5
    for a, b in ((soft, None), (xd, soft[:m])):
        out = kern(a) if b is None else kern(a, b)
        assert isinstance(out, DenseLinearOperator)
        b = a if b is None else b
        want = g.kernels.hamming_dense(a.double().cpu(), b.double().cpu(), v, 0.8, 1.7) * 1.2
        assert rel_err(operators.to_dense(out), want) < 1e-5
    tl = _cloud(gen, 50, 129, 2, _parents(gen, 129, 2))
    k2 = g.kernels.HammingIMQKernel(vocab_size=2).to(dev)
    k2.alpha, k2.beta = 0.8, 1.7
    o129 = k2(one_hot(tl, 2).to(dev))
    assert isinstance(o129, DenseLinearOperator) and rel_err(operators.to_dense(o129), hamming_k(hamming_counts(tl), 0.8, 1.7)) < 1e-5
    assert isinstance(k2(one_hot(tl[:, :128], 2).to(dev)), FusedKernelLinearOperator)
    k64 = g.kernels.HammingIMQKernel(vocab_size=v).to(dev).double()
    k64.alpha, k64.beta = 0.8, 1.7
    o64_ = k64(xd.double())
    assert isinstance(o64_, DenseLinearOperator) and rel_err(operators.to_dense(o64_), hamming_k(hamming_counts(tok), 0.8, 1.7)) < 1e-12


def test_sum_with_a_matern_kernel_on_covariates(dev):
    """ScaleKernel(HammingIMQKernel(active_dims=sequence columns)) + ScaleKernel(MaternKernel(active_dims=covariate columns)): the marginal log
    likelihood and its gradients against dense float64 autograd within the model-level bounds, on both branches, whichever sum operator carries it."""
    import gpytorch_amd as g
    from tests.util import make_data

    n, t, v, dc = 300, 17, 4, 2
    gen = torch.Generator().manual_seed(3)
    tok = _cloud(gen, n, t, v, _parents(gen, t, v))
    Xc, y = make_data(n, dc, seed=4)
    Xc, y = Xc.float().double(), y.float().double()
    y = y + 0.5 * (tok[:, 2] == tok[0, 2]).double()
    X = torch.cat([one_hot(tok, v).double(), Xc], dim=1)
    seq, cov = list(range(t * v)), [t * v, t * v + 1]
    vals = dict(alpha=1.1, beta=1.4, os_h=0.9, ls=0.6, os_m=0.7, noise=0.1)
    leaves = {k: torch.tensor(x, dtype=torch.float64, requires_grad=True) for k, x in vals.items()}
    r = (Xc.unsqueeze(1) - Xc.unsqueeze(0)).norm(dim=-1) * math.sqrt(5.0) / leaves["ls"]
    Km = (1 + r + r * r / 3) * torch.exp(-r)
    Khat = leaves["os_h"] * hamming_k(hamming_counts(tok), leaves["alpha"], leaves["beta"]) + leaves["os_m"] * Km + leaves["noise"] * torch.eye(n, dtype=torch.float64)
    ref = OG.dense_log_prob(Khat, y) / n
    order = ["alpha", "beta", "os_h", "ls", "os_m", "noise"]
    gref = torch.autograd.grad(ref, [leaves[k] for k in order])
    want = torch.tensor([float(gr) * _sp(vals[k] - (1e-4 if k == "noise" else 0.0)) for gr, k in zip(gref, order)], dtype=torch.float64)

    class M(g.models.ExactGP):
        def __init__(self, x, yy, lik):
            super().__init__(x, yy, lik)
            self.mean_module = g.means.ZeroMean()
            self.covar_module = (g.kernels.ScaleKernel(g.kernels.HammingIMQKernel(vocab_size=v, active_dims=seq))
                                 + g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5, active_dims=cov)))

        def forward(self, x):
            return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    for branch in ("cholesky", "bbmm"):
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X.float().to(dev), y.float().to(dev), lik).to(dev)
        kh, km = m.covar_module.kernels
        kh.base_kernel.alpha, kh.base_kernel.beta, kh.outputscale = vals["alpha"], vals["beta"], vals["os_h"]
        km.base_kernel.lengthscale, km.outputscale, lik.noise = vals["ls"], vals["os_m"], vals["noise"]
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
        got = torch.tensor([float(kh.base_kernel.raw_alpha.grad), float(kh.base_kernel.raw_beta.grad), float(kh.raw_outputscale.grad),
                            float(km.base_kernel.raw_lengthscale.grad.sum()), float(km.raw_outputscale.grad), float(lik.noise_covar.raw_noise.grad.sum())],
                           dtype=torch.float64)
        e_v, e_g = abs(float(val.detach()) - float(ref)) / max(1.0, abs(float(ref))), float((got - want).norm() / want.norm())
        print("sum mll", branch, type(m.covar_module(m.train_inputs[0])).__name__, e_v, e_g, got, want)
        assert e_v < tol_v, (branch, float(val), float(ref))
        assert e_g < tol_g, (branch, got, want)
