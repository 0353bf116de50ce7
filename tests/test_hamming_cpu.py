"""CPU: the inverse-multiquadric Hamming kernel (``kernels.HammingIMQKernel``, the native family ``"hamming"`` over packed tokens) -- ``hamming_dense``
against the reference's own outputs (tests/golden/hamming_values.npz, made by tests/golden/make_hamming_golden.py), the packed rows of
``families.hamming_prep``, the torch restatement ``families.hamming_cov`` on them, the rule ``hamming_native``, the routing of ``forward``, the chain
rule of ``functions._hamming_hyper_grads``, the family record and the ABI's refusals with null buffers (nothing launches)."""
import os

import numpy as np
import pytest
import torch

import gpytorch_amd as g
from gpytorch_amd import backend as B
from gpytorch_amd import operators
from gpytorch_amd.kernels import HammingIMQKernel, ScaleKernel, hamming_dense, hamming_native
from tests.hamming_ref import hamming_counts, hamming_grad_sums, hamming_k, hamming_kt, one_hot, random_tokens, tokens
from tests.test_ski_cpu import _Fake

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hamming_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files if k.endswith("_x1")})


def _case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


def _abs_err(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def _vocab(name):
    return int(name[name.index("v") + 1:-3])


def _prepared(tok, v, alpha, beta):
    rows, valid = B.hamming_prep(one_hot(tok, v), v)
    assert bool(valid)
    par = B.HammingParams(tok.shape[1], v, alpha, beta)
    return B.PreparedPoints(rows, tok.shape[0], par.width, rows.shape[1], "hamming", par)


def test_fixture_covers_the_cases():
    shapes = {(GOLD[f"{c}_x1"].shape[1] // _vocab(c), _vocab(c)) for c in CASES}
    assert shapes == {(1, 2), (3, 4), (5, 20)} and len(CASES) == 12
    assert all(12 <= GOLD[f"{c}_x1"].shape[0] <= 17 for c in CASES)
    assert {GOLD[f"{c}_x1"].dtype for c in CASES} == {np.dtype("float32"), np.dtype("float64")}
    assert {c[-3] for c in CASES} == {"e", "t"}


@pytest.mark.parametrize("name", CASES)
def test_hamming_dense_matches_the_reference(name):
    """``kernels.hamming_dense`` and the kernel's dense branch against the reference's own outputs: 1e-12 in float64, 1e-6 in float32, absolute -- K,
    ``diag=True`` of one input and of two.  The values are ratios of small integers raised to beta; so is the float64 oracle on tokens."""
    c = _case(name)
    f64 = c["x1"].dtype == np.float64
    dt, tol, v = (torch.float64 if f64 else torch.float32), (1e-12 if f64 else 1e-6), _vocab(name)
    x1, x2 = torch.as_tensor(c["x1"]), torch.as_tensor(c["x2"])
    alpha, beta = torch.as_tensor(c["alpha"]), torch.as_tensor(c["beta"])
    k = min(x1.shape[0], x2.shape[0])
    with torch.no_grad():
        K = hamming_dense(x1, x2, v, alpha, beta)
        errs = [_abs_err(K, c["K"]), _abs_err(hamming_dense(x1, x1, v, alpha, beta, diag=True), c["diag_same"]),
                _abs_err(hamming_dense(x1[:k], x2[:k], v, alpha, beta, diag=True), c["diag_pair"])]
        oracle = hamming_k(hamming_counts(tokens(x1, v), tokens(x2, v)), alpha.double(), beta.double())
        errs.append(_abs_err(oracle, c["K"]))
        print(name, errs)
        assert K.dtype == dt and K.shape == c["K"].shape and c["diag_same"].shape == (x1.shape[0],) and max(errs) < tol, errs
        kern = HammingIMQKernel(vocab_size=v).to(dt)
        kern.alpha, kern.beta = alpha, beta
        if f64:   # (float32 one-hot inputs take the native operator, which needs the device: tests/test_gpu_hamming.py)
            out = kern(x1, x2)
            assert isinstance(out, operators.DenseLinearOperator) and _abs_err(operators.to_dense(out), c["K"]) < tol
        assert _abs_err(kern(x1, diag=True), c["diag_same"]) < tol and _abs_err(kern(x1[:k], x2[:k], diag=True), c["diag_pair"]) < tol


def test_prepared_rows():
    """``hamming_prep`` on hand-built rows: the byte of a position is token + 1, the padding byte is 1, four positions per dword; the widths; the
    validity flag; every dword a normal finite float."""
    v = 5
    tok = torch.tensor([[0, 4, 2, 2, 1, 3], [4, 4, 4, 4, 4, 4]])
    rows, valid = B.hamming_prep(one_hot(tok, v), v)
    assert rows.dtype == torch.float32 and rows.shape == (2, 4) and valid.dtype == torch.bool and valid.dim() == 0 and bool(valid)
    by = rows.view(torch.int8)
    assert by.shape == (2, 16) and torch.equal(by[:, :6], (tok + 1).to(torch.int8)) and torch.equal(by[:, 6:], torch.ones(2, 10, dtype=torch.int8))
    assert int(rows.view(torch.int32)[0, 0]) == 1 | (5 << 8) | (3 << 16) | (3 << 24)            # position p at byte p % 4 of dword p // 4
    for t, w in ((1, 4), (16, 4), (17, 8), (32, 8), (33, 16), (64, 16), (65, 32), (128, 32)):
        tk = random_tokens(3, t, 126, 40 + t)
        r, ok = B.hamming_prep(one_hot(tk, 126), 126)
        assert r.shape == (3, w) and B.hamming_width(t) == w and bool(ok)
        b = r.view(torch.int8)
        assert torch.equal(b[:, :t], (tk + 1).to(torch.int8)) and bool((b[:, t:] == 1).all()) and int(b.min()) >= 1
        # no prepared dword is zero, subnormal, infinite or NaN when read as float32
        assert bool(torch.isfinite(r).all()) and bool((r.abs() >= torch.finfo(torch.float32).tiny).all())
    tk = torch.full((2, 128), 125)                                                                  # the largest byte everywhere: 126 = 0x7e
    r, _ = B.hamming_prep(one_hot(tk, 126), 126)
    assert bool(torch.isfinite(r).all()) and bool((r.view(torch.int8) == 126).all())
    # the validity flag: a two-hot position, a zero position, a 0.5 entry
    x = one_hot(tok, v)
    for edit in (lambda z: z.__setitem__((0, 3), 1.0), lambda z: z.__setitem__((1, 4), 0.0), lambda z: z.__setitem__((0, 1), 0.5),
                 lambda z: (z.__setitem__((0, 1), 0.5), z.__setitem__((0, 0), 0.5))):
        z = x.clone()
        edit(z)
        r, ok = B.hamming_prep(z, v)
        assert not bool(ok) and r.shape == (2, 4)
    with pytest.raises(ValueError):
        B.hamming_prep(x.double(), v)
    with pytest.raises(ValueError):
        B.hamming_prep(x.reshape(1, 2, -1), v)
    with pytest.raises(ValueError):
        B.hamming_prep(x, 4)
    with pytest.raises(ValueError):
        B.hamming_prep(one_hot(torch.zeros(2, 129, dtype=torch.long), 2), 2)
    with pytest.raises(ValueError):
        B.hamming_prep(one_hot(torch.zeros(2, 3, dtype=torch.long), 127), 127)


def test_mismatch_count_identity():
    """popcount(((a ^ b) + 0x7f7f7f7f) & 0x80808080) counts the differing bytes of two dwords whose bytes lie in 1..127 -- the kernels' instruction
    sequence restated on integers, every pair of byte values in one lane and random dwords."""
    vals = torch.arange(1, 128, dtype=torch.int64)
    a, b = vals.unsqueeze(1), vals.unsqueeze(0)
    for shift in (0, 8, 16, 24):
        x = (((a << shift) ^ (b << shift)) + 0x7F7F7F7F) & 0x80808080
        assert int(x.max()) < 2 ** 32 and torch.equal(x != 0, a != b) and torch.equal(x, (a != b).to(torch.int64) << (shift + 7))
    gen = torch.Generator().manual_seed(1)
    p, q = torch.randint(1, 128, (4000, 4), generator=gen), torch.randint(1, 128, (4000, 4), generator=gen)
    q[::3, 1], q[::5, 3] = p[::3, 1], p[::5, 3]
    pack = lambda t: t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)
    x = ((pack(p) ^ pack(q)) + 0x7F7F7F7F) & 0x80808080
    cnt = sum((x >> s) & 1 for s in (7, 15, 23, 31))
    assert int(x.max()) < 2 ** 32 and torch.equal(cnt, (p != q).sum(1))


def test_hamming_cov_on_prepared_rows():
    """``families.hamming_cov`` (float32, the kernels' arithmetic) against float64 from the raw one-hot inputs.  The bound, from the arithmetic: with
    e = 2^-24, s = fl(c fl(1 / alpha)) and u = fl(1 + s) carry a relative error <= 3 e; log2 and exp2 are within one ulp; the exponent
    t = beta log2(u) then carries t (1 ulp of log2 + the rounding of beta + of the product = 3 e) + beta 3 e / ln 2, which exp2 amplifies by ln 2:
    |dk| <= k t ln2 3 e + k beta 3 e + k e <= (0.37 * 3 + 3 beta + 1) e since k t ln 2 = k ln(1 / k) <= 1 / e and k <= 1 -- under (3 + 3 beta) 2^-24,
    asserted with a factor two for library log2 / exp2 that round within two ulp: (3 + 3 beta) 2^-23."""
    for idx, (t, v, alpha, beta) in enumerate(((1, 2, 0.3, 0.5), (16, 20, 1.7, 3.0), (17, 4, 3.0, 1.1), (65, 20, 0.9, 2.3), (128, 126, 0.31, 2.9))):
        tok1 = random_tokens(19, t, v, 100 + idx)
        tok2 = random_tokens(23, t, v, 200 + idx, close_to=tok1)
        p1, p2 = _prepared(tok1, v, alpha, beta), _prepared(tok2, v, alpha, beta)
        x1, x2 = one_hot(tok1, v, torch.float64), one_hot(tok2, v, torch.float64)
        c = (t - x1 @ x2.t()).clamp_min(0)                                      # float64 from the raw one-hot inputs
        assert torch.equal(c, hamming_counts(tok1, tok2))
        want = hamming_kt(c, alpha, beta)
        bound = (3 + 3 * beta) * 2.0 ** -23
        got = B.hamming_cov(p1, p2)
        err = _abs_err(got, want)
        print("hamming_cov", t, v, alpha, beta, err, bound)
        assert got.dtype == torch.float32 and got.shape == (19, 23) and err < bound
        assert bool((got[c == 0] == 1.0).all()) and int((c == 0).sum()) > 0      # c = 0: an exact one
        S = 1.7
        assert _abs_err(B.kernel_dense(p1, p2, torch.tensor([S])), S * want) < S * bound
        rows = torch.tensor([4, 0, 18])
        assert _abs_err(B.kernel_rows(p1, rows, p2), want[rows]) < bound
        assert _abs_err(B.kernel_diag(_prepared(tok1, v, alpha, beta), _prepared(tok2[:19], v, alpha, beta)), want[:, :19].diagonal()) < bound
        assert torch.equal(B.kernel_diag(p1, p1), torch.ones(19)) and torch.equal(B.kernel_dense(p1, p1).diagonal(), torch.ones(19))
        # policy: one kernel, never culled, no Gram-form derivative, no float64 fused path, planned as the Gibbs family at width min(W, 8)
        for tc in (1, 5, 33, 65):
            assert B.kv_flags(p1, p2, tc) == B.KV_SPLIT
        with g.settings.far_pair_cutoff(1e-3):
            assert B.far_cull(p1, p2) is None
        assert not B.grad_gram_ok(p1, p2) and not B.f64_widenable(p1)
        assert B.kv_plan("hamming", 2000, 2000, p1.d, 11, B.KV_SPLIT, 2000) == B.kv_plan("gibbs", 2000, 2000, min(p1.d, 8), 11, B.KV_SPLIT, 2000)


def test_hamming_native_truth_table():
    def kern(v=4, **kw):
        return HammingIMQKernel(vocab_size=v, **kw)

    x = _Fake((10, 12))
    assert hamming_native(kern(), x) and hamming_native(kern(), x, _Fake((7, 12)))
    assert hamming_native(kern(), _Fake((10, 12), device="cpu"))                                  # pure: never looks at the device
    # float32 inputs and parameters
    assert not hamming_native(kern(), _Fake((10, 12), dtype=torch.float64)) and not hamming_native(kern(), x, _Fake((7, 12), dtype=torch.float64))
    assert not hamming_native(kern().double(), x)
    half = kern()
    half.raw_beta.data = half.raw_beta.data.double()
    assert not hamming_native(half, x)
    # no batch shape anywhere, no last_dim_is_batch
    assert not hamming_native(kern(), _Fake((2, 10, 12))) and not hamming_native(kern(), x, _Fake((2, 7, 12)))
    assert not hamming_native(kern(batch_shape=torch.Size([2])), x) and not hamming_native(kern(), x, last_dim_is_batch=True)
    # the width a multiple of V, the same for both clouds
    assert not hamming_native(kern(v=5), x) and not hamming_native(kern(), x, _Fake((7, 8)))
    # T <= 128 and V <= 126
    assert hamming_native(kern(v=2), _Fake((10, 2 * 128))) and not hamming_native(kern(v=2), _Fake((10, 2 * 129)))
    assert hamming_native(kern(v=126), _Fake((10, 126 * 3))) and not hamming_native(kern(v=127), _Fake((10, 127 * 3)))
    assert hamming_native(kern(v=126), _Fake((10, 126 * 128))) and hamming_native(kern(v=1), _Fake((10, 1)))
    # inputs without requires_grad
    assert not hamming_native(kern(), _Fake((10, 12), requires_grad=True)) and not hamming_native(kern(), x, _Fake((7, 12), requires_grad=True))


def test_forward_routing_and_reference_behaviours():
    v, t = 4, 3
    tok, tok2 = random_tokens(15, t, v, 1), random_tokens(9, t, v, 2)
    x, x2 = one_hot(tok, v), one_hot(tok2, v)
    kern = HammingIMQKernel(vocab_size=v)
    kern.alpha, kern.beta = 0.8, 1.5
    assert tuple(kern.raw_alpha.shape) == (1,) and abs(float(kern.alpha.detach()) - 0.8) < 1e-6 and abs(float(kern.beta.detach()) - 1.5) < 1e-6
    assert tuple(HammingIMQKernel(3, batch_shape=torch.Size([2])).raw_beta.shape) == (2, 1) and not kern.has_lengthscale
    k0 = (1.8 / 0.8) ** 1.5
    # ONE fused operator of kind "hamming": ones in the lengthscale slot, the differentiable k0 in the outputscale slot, theta = [alpha, beta]
    for a, b in ((x, None), (x, x2)):
        op = kern(a) if b is None else kern(a, b)
        assert isinstance(op, operators.FusedKernelLinearOperator) and op.spec.kind == "hamming" and op.spec.code == v and op.spec.shift is None
        assert op.shape == (15, 15 if b is None else 9) and torch.equal(op.lengthscale, torch.ones(1, 1)) and not op.lengthscale.requires_grad
        assert abs(float(op.outputscale.detach()) - k0) < 1e-5 and op.outputscale.requires_grad and tuple(op.outputscale.shape) == (1,)
        assert tuple(op.spec.param.shape) == (2,) and op.spec.param.requires_grad and _abs_err(op.spec.param.detach(), torch.tensor([0.8, 1.5])) < 1e-6
    ga, gb = torch.autograd.grad(op.outputscale.sum(), [kern.raw_alpha, kern.raw_beta])
    assert float(ga) < 0 < float(gb)                                                              # k0 falls with alpha and grows with beta
    sk = ScaleKernel(kern)
    sk.outputscale = 1.3
    ops = sk(x, x2)
    assert isinstance(ops, operators.FusedKernelLinearOperator) and ops.spec.kind == "hamming" and abs(float(ops.outputscale.detach()) - 1.3 * k0) < 1e-5
    code, theta = ops.spec.param_value()
    assert code == v and not theta.requires_grad
    # diag: equal inputs -> k0 expanded to [n] (no launch), two different inputs -> the elementwise value
    dg = kern(x, diag=True)
    assert dg.shape == (15,) and torch.allclose(dg.detach(), torch.full((15,), k0)) and dg.requires_grad
    want = hamming_k((tok[:9] != tok2).sum(-1).double(), 0.8, 1.5)
    assert _abs_err(kern(x[:9], x2, diag=True).detach(), want) < 1e-6
    # a width not divisible by V: RuntimeError, as the reference's view raises
    with pytest.raises(RuntimeError):
        kern(torch.rand(5, 10))
    with pytest.raises(RuntimeError):
        kern(torch.rand(5, 10), diag=True)
    # declined calls: DenseLinearOperator of hamming_dense -- not one-hot, T = 129, V = 127, float64, a batch, inputs that require grad
    soft = x.clone()
    soft[0, :4] = torch.tensor([0.5, 0.5, 0.0, 0.0])
    out = kern(soft, x2)
    assert isinstance(out, operators.DenseLinearOperator)
    assert _abs_err(operators.to_dense(out).detach(), hamming_dense(soft.double(), x2.double(), v, 0.8, 1.5)) < 1e-5
    assert isinstance(kern(x, soft[:9]), operators.DenseLinearOperator)
    long = one_hot(random_tokens(6, 129, 2, 3), 2)
    k2 = HammingIMQKernel(vocab_size=2)
    assert isinstance(k2(long), operators.DenseLinearOperator) and isinstance(k2(long[:, : 2 * 128]), operators.FusedKernelLinearOperator)
    assert isinstance(HammingIMQKernel(127)(one_hot(random_tokens(6, 2, 127, 4), 127)), operators.DenseLinearOperator)
    assert isinstance(HammingIMQKernel(126)(one_hot(random_tokens(6, 2, 126, 4), 126)), operators.FusedKernelLinearOperator)
    k64 = HammingIMQKernel(vocab_size=v).double()
    k64.alpha, k64.beta = 0.8, 1.5
    o64 = k64(x.double())
    assert isinstance(o64, operators.DenseLinearOperator) and _abs_err(operators.to_dense(o64).detach(), hamming_k(hamming_counts(tok), 0.8, 1.5)) < 1e-12
    kb = HammingIMQKernel(vocab_size=v, batch_shape=torch.Size([2]))
    assert tuple(kb(x.expand(2, *x.shape), diag=True).shape) == (2, 15)
    xg = x.clone().requires_grad_(True)
    og = kern(xg)
    assert isinstance(og, operators.DenseLinearOperator)
    operators.to_dense(og).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and kern.raw_alpha.grad is not None and kern.raw_beta.grad is not None
    # the validity flag is read once per source tensor
    from gpytorch_amd import kernels as K

    K._HAMMING_ONE_HOT.clear()
    calls = []
    real = B.hamming_prep
    try:
        B.hamming_prep = lambda *a: (calls.append(1), real(*a))[1]
        kern(x), kern(x), kern(x, x2), kern(x, x2)
    finally:
        B.hamming_prep = real
    assert len(calls) == 2
    x[0, 0] = x[0, 0]                                                                               # a new version of the tensor: read again
    assert isinstance(kern(x), operators.FusedKernelLinearOperator)


def test_constraints_and_priors_reach_alpha_and_beta():
    from gpytorch_amd.constraints import Interval
    from gpytorch_amd.priors import GammaPrior, NormalPrior

    kern = HammingIMQKernel(vocab_size=4, alpha_prior=GammaPrior(2.0, 1.0), alpha_constraint=Interval(0.1, 5.0), beta_prior=NormalPrior(1.0, 0.5),
                            beta_constraint=Interval(0.2, 4.0))
    assert type(kern.raw_alpha_constraint) is Interval and type(kern.raw_beta_constraint) is Interval
    assert abs(float(kern.alpha) - 2.55) < 1e-5 and abs(float(kern.beta) - 2.1) < 1e-5       # raw 0 under an Interval: its midpoint
    kern.alpha, kern.beta = 0.7, 3.0
    assert abs(float(kern.alpha) - 0.7) < 1e-5 and abs(float(kern.beta) - 3.0) < 1e-5
    names = {name for name, *_ in kern.named_priors()}
    assert names == {"alpha_prior", "beta_prior"}
    for name, _, prior, closure, setting in kern.named_priors():
        assert abs(float(closure(kern)) - (0.7 if name == "alpha_prior" else 3.0)) < 1e-5
        setting(kern, 1.25)
    assert abs(float(kern.alpha) - 1.25) < 1e-5 and abs(float(kern.beta) - 1.25) < 1e-5
    plain = HammingIMQKernel(vocab_size=4)
    assert type(plain.raw_alpha_constraint).__name__ == "Positive" and type(plain.raw_beta_constraint).__name__ == "Positive"
    assert not list(plain.named_priors())


def test_hyper_grads_from_sums():
    """``functions._hamming_hyper_grads`` on sums handed in (nothing launches), the three sums computed in float64 torch, against float64 autograd of
    sum W s k~ through a ``ScaleKernel`` around the kernel (its dense float64 branch): alpha and beta receive their gradient through the
    learnable-parameter slot at fixed s PLUS through s = outputscale k0(alpha, beta); the outer scale through s alone.  1e-10."""
    from gpytorch_amd.functions import _hamming_hyper_grads, hyper_grads

    v, t = 6, 7
    tok1, tok2 = random_tokens(11, t, v, 5), random_tokens(8, t, v, 6, close_to=random_tokens(11, t, v, 5))
    W = torch.randn(11, 8, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    sk = ScaleKernel(HammingIMQKernel(vocab_size=v)).double()
    sk.base_kernel.alpha, sk.base_kernel.beta, sk.outputscale = 0.9, 2.2, 1.3
    raws = [sk.base_kernel.raw_alpha, sk.base_kernel.raw_beta, sk.raw_outputscale]
    dense = sk(one_hot(tok1, v, torch.float64), one_hot(tok2, v, torch.float64))
    assert isinstance(dense, operators.DenseLinearOperator)
    want = torch.autograd.grad((W * operators.to_dense(dense)).sum(), raws)
    alpha, beta = sk.base_kernel.alpha, sk.base_kernel.beta
    slot = (sk.outputscale * ((1 + alpha) / alpha).pow(beta)).reshape(1)             # what rides in the operator's outputscale slot
    theta = torch.cat([alpha.reshape(1), beta.reshape(1)])
    sums = hamming_grad_sums(hamming_counts(tok1, tok2), alpha, beta, W)
    p1, p2 = _prepared(tok1, v, alpha, beta), _prepared(tok2, v, alpha, beta)
    ones = torch.ones(1, 1, dtype=torch.float64)
    d_ls, d_os, d_theta = _hamming_hyper_grads(p1, p2, ones, slot.detach(), None, None, False, theta.detach(), sums=sums)
    assert torch.equal(d_ls, torch.zeros(1, 1, dtype=torch.float64)) and d_os.shape == (1,) and d_theta.shape == (2,)
    got = torch.autograd.grad([slot, theta], raws, grad_outputs=[d_os, d_theta])
    errs = [abs(float(a) - float(b)) for a, b in zip(got, want)]
    print("hyper grads", errs, [float(w) for w in want])
    assert max(errs) < 1e-10
    # without a learnable-parameter slot: two values; without an outputscale: s = 1
    assert len(_hamming_hyper_grads(p1, p2, ones, slot.detach(), None, None, False, None, sums=sums)) == 2
    _, none, d1 = _hamming_hyper_grads(p1, p2, ones, None, None, None, False, theta.detach(), sums=sums)
    assert none is None and _abs_err(d1, torch.stack([-sums[1] / alpha.detach().reshape(()), sums[2]])) < 1e-14
    with pytest.raises(RuntimeError, match="'hamming'"):
        hyper_grads(p1, p2, ones, None, None, None, want_x1=True)
    with pytest.raises(RuntimeError, match="'hamming'"):
        hyper_grads(p1, p2, ones, None, None, None, want_x2=True)


def test_family_record_and_id():
    from gpytorch_amd.functions import KernelSpec, _OWN_HYPER_GRADS

    f = B.FAMILIES["hamming"]
    assert B.HAMMING_KIND_ID == 12 and f.id == 12 and "hamming" not in B.KIND_IDS and len(B.KIND_IDS) == 11
    assert f.name == "hamming" and f.plan_kind == "gibbs" and f.one_kernel and not f.has_f64 and not f.widenable and not f.stackable
    assert f.cov is B.hamming_cov and f.launch is not None and f.grad_param is None and "hamming" in _OWN_HYPER_GRADS
    assert [f.plan_dims(w) for w in (4, 8, 16, 32)] == [4, 8, 8, 8] and B.FAMILIES["gibbs"].plan_dims(8) == 8
    theta = torch.tensor([0.5, 2.0], requires_grad=True)
    code, th = KernelSpec("hamming", code=4, param=theta).param_value()
    assert code == 4 and torch.equal(th, theta.detach()) and not th.requires_grad
    x = one_hot(random_tokens(5, 3, 4, 0), 4)
    par, lead, rows = f.prepare(x, None, (4, theta))
    assert (par.t, par.v, par.width) == (3, 4, 4) and lead is None and rows.shape == (5, 4) and rows.dtype == torch.float32
    assert par.alpha.dtype == par.beta.dtype == torch.float64 and float(par.alpha) == 0.5 and float(par.beta) == 2.0
    assert par.inv_alpha == 2.0 and par.beta_f == 2.0 and isinstance(par.inv_alpha, float)
    third = B.HammingParams(3, 4, 3.0, 0.1)
    assert third.inv_alpha == float(torch.tensor(1.0 / 3.0, dtype=torch.float32)) and third.beta_f == float(torch.tensor(0.1, dtype=torch.float32))
    again, _, _ = f.prepare(x, None, par)
    assert again is par
    for bad in (None, (5, theta), (4, torch.tensor([0.0, 1.0])), (4, torch.tensor([1.0, float("inf")]))):
        with pytest.raises(ValueError):
            f.prepare(x, None, bad)
    with pytest.raises(ValueError):
        f.prepare(x.double(), None, (4, theta))                        # float32 only
    with pytest.raises(ValueError):
        f.prepare(x.reshape(1, 5, 12), None, (4, theta))                # no batches
    with pytest.raises(ValueError):
        f.prepare(one_hot(random_tokens(5, 129, 2, 0), 2), None, (2, theta))
    for name in ("HammingIMQKernel", "hamming_native", "hamming_dense"):
        assert name in g.kernels.__all__ and hasattr(g.kernels, name)


def _err(h):
    return h.gpamd_last_error()


def test_abi_header_exports_and_refusals_before_any_launch():
    import ctypes as C

    from gpytorch_amd._lib import SIGNATURES, lib

    h = lib()
    assert h.gpamd_abi_version() == 5                               # additive: the version stands
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gpamd.h")).read()
    assert "GPAMD_HAMMING = 12" in header and "KIND_HAMMING = 12" in open(os.path.join(root, "gpytorch_amd", "csrc", "common.hpp")).read()
    for name in ("gpamd_kv_hamming_partials_f32", "gpamd_kv_hamming_grad_workspace_doubles", "gpamd_kv_hamming_grad_f32"):
        assert name in header and name in SIGNATURES and hasattr(h, name)
    tail = (None, 300, None, 300, None, 300, 11, None, 300, 1, 384, None, None)            # X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk, done, stream
    gtail = (None, 300, None, 300, None, 300, None, 300, 8, None, None, 0, None)           # X1p, n, X2p, m, Lt, ldl, Rt, ldr, t, out, ws, ws_doubles, stream
    for w in (0, 1, 5, 12, 24, 64, -4):
        assert h.gpamd_kv_hamming_partials_f32(w, 1.0, 1.0, *tail) == -2 and _err(h).startswith(b"kv_hamming:") and b"4, 8, 16 or 32" in _err(h)
        assert h.gpamd_kv_hamming_grad_f32(w, 1.0, 1.0, *gtail) == -2 and _err(h).startswith(b"kv_hamming_grad:") and b"4, 8, 16 or 32" in _err(h)
        assert h.gpamd_kv_hamming_grad_workspace_doubles(300, 300, 8, w) == 0
    for ia, be in ((0.0, 1.0), (-1.0, 1.0), (1.0, 0.0), (float("inf"), 1.0), (1.0, float("nan"))):
        assert h.gpamd_kv_hamming_partials_f32(8, ia, be, *tail) == -1 and _err(h).startswith(b"kv_hamming:") and b"positive and finite" in _err(h)
        assert h.gpamd_kv_hamming_grad_f32(8, ia, be, *gtail) == -1 and _err(h).startswith(b"kv_hamming_grad:") and b"positive and finite" in _err(h)
    # a valid call gets as far as the shape checks of the shared launch code / the null-pointer check of the derivative
    for w in (4, 8, 16, 32):
        assert h.gpamd_kv_hamming_partials_f32(w, 2.0, 1.5, *(tail[:5] + (302,) + tail[6:])) == -1 and b"leading dimensions" in _err(h)
        assert h.gpamd_kv_hamming_partials_f32(w, 2.0, 1.5, *(tail[:6] + (0,) + tail[7:])) == -1 and b"bad shape" in _err(h)
        assert h.gpamd_kv_hamming_grad_f32(w, 2.0, 1.5, *gtail) == -1 and _err(h).startswith(b"kv_hamming_grad: bad arguments")
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    ok = [p, 300, p, 200, p, 300, p, 200, 9, p, p, 1 << 40, None]
    need = h.gpamd_kv_hamming_grad_workspace_doubles(300, 200, 9, 16)
    assert need > 0 and need % 3 == 0 and need == h.gpamd_kv_hamming_grad_workspace_doubles(300, 200, 9, 4)
    for i in (0, 2, 4, 6, 9, 10):                                                           # each pointer null in turn
        a = list(ok)
        a[i] = None
        assert h.gpamd_kv_hamming_grad_f32(16, 2.0, 1.5, *a) == -1 and _err(h).startswith(b"kv_hamming_grad: bad arguments")
    for i, val in ((1, 0), (3, 0), (8, 0), (5, 299), (7, 199)):                             # n, m, t, ldl, ldr
        a = list(ok)
        a[i] = val
        assert h.gpamd_kv_hamming_grad_f32(16, 2.0, 1.5, *a) == -1 and _err(h).startswith(b"kv_hamming_grad: bad arguments")
    a = list(ok)
    a[11] = need - 1
    assert h.gpamd_kv_hamming_grad_f32(16, 2.0, 1.5, *a) == -3 and _err(h).startswith(b"kv_hamming_grad:") and b"workspace" in _err(h)
    # the plan is the Gibbs family's; every entry point that takes a kind refuses 12 as the unknown kind it was
    HAM, SPLIT = 12, 8
    assert h.gpamd_kv_plan(10, 2000, 2000, 8, 11, SPLIT, 2000, None, None, None) == 0
    assert h.gpamd_kv_plan(HAM, 2000, 2000, 8, 11, SPLIT, 2000, None, None, None) == -1
    assert h.gpamd_kv_partials_f32(HAM, 0.0, None, 300, None, 300, 8, None, None, 300, 11, None, 300, 1, 384, SPLIT, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_prep_points_f32(HAM, 0.0, None, 5, 3, 3, None, 1, None, None, 4, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_dense_f32(HAM, 0.0, None, 10, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_rows_f32(HAM, 0.0, None, None, 3, None, 10, 4, None, None, 12, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kernel_diag_f32(HAM, 0.0, None, None, 10, 4, None, None, None) == -1 and b"unknown kind" in _err(h)
    assert h.gpamd_kv_grad_f32(HAM, None, 300, None, 300, 4, None, 300, None, 300, 9, 0, None, None, 0, None) == -1
    assert h.gpamd_kv_f32(HAM, 0.0, None, 300, None, 300, 3, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, SPLIT, None) == -1
    assert h.gpamd_pivoted_cholesky_f32(HAM, 0.0, None, 100, 4, None, 5, 1e-3, None, 100, None, None, None, None) == -1
