"""CPU: the spectral-mixture family off the device -- the reference's recorded values (tests/golden/sm_values.npz, made by executing the reference's
forward) against the float64 restatement (tests/sm_ref.py) and ``kernels.sm_dense``; the chain rule from the sums A, B, C against autograd; the module
surface; the recognition rule ``kernels.sm_native``; the dense branch of what it declines; the C ABI's refusals (before any launch: no device needed)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import sm_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sm_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})


def _case(name):
    t = {k: torch.from_numpy(np.asarray(GOLD[f"{name}_{k}"])) for k in ("x1", "x2", "w", "mu", "sigma", "K")}
    return t, bool(GOLD[f"{name}_diag"]), bool(GOLD[f"{name}_ldb"])


def test_golden_covers_the_envelope():
    seen = set()
    for name in CASES:
        t, diag, ldb = _case(name)
        seen.add((t["x1"].shape[1], t["w"].numel(), t["K"].dtype, diag, ldb, t["x1"].shape == t["x2"].shape and bool((t["x1"] == t["x2"]).all())))
    assert {s[0] for s in seen} == {1, 2, 3} and {s[1] for s in seen} == {1, 3, 4, 8}
    assert {s[2] for s in seen} == {torch.float32, torch.float64} and any(s[3] for s in seen) and any(s[4] for s in seen)
    assert any(s[5] for s in seen) and any(not s[5] for s in seen)


@pytest.mark.parametrize("name", CASES)
def test_golden_restatement_and_dense_agree(name):
    from gpytorch_amd.kernels import sm_dense

    t, diag, ldb = _case(name)
    tol = 1e-12 if t["K"].dtype == torch.float64 else 1e-5
    x1, x2, w, mu, sigma = t["x1"], t["x2"], t["w"], t["mu"], t["sigma"]
    dense = sm_dense(x1, x2, w, mu, sigma, diag=diag, last_dim_is_batch=ldb)
    assert dense.shape == t["K"].shape and dense.dtype == t["K"].dtype
    mu2, sg2 = mu.reshape(mu.shape[0], -1), sigma.reshape(sigma.shape[0], -1)
    if ldb:      # the per-dimension factors as batch members: each is the one-dimensional kernel of its column
        ref = torch.stack([R.sm_cov(x1[:, j : j + 1], x2[:, j : j + 1], w, mu2[:, j : j + 1], sg2[:, j : j + 1]) for j in range(x1.shape[1])])
    else:
        ref = R.sm_cov(x1, x2, w, mu2, sg2)
        ref = ref.diagonal() if diag else ref
    scale = float(t["K"].abs().max())
    for what, a in (("golden vs restatement", ref), ("golden vs sm_dense", dense)):
        err = float((a.double() - t["K"].double()).abs().max()) / scale
        assert err < tol, (name, what, err)
    if not (diag or ldb) and x1.shape == x2.shape and bool((x1 == x2).all()):
        assert torch.allclose(ref.diagonal(), (w.double().sum() ** x1.shape[1]).expand(x1.shape[0]), rtol=1e-13)    # k(x, x) = Wsum^d


@pytest.mark.parametrize("qd", [(1, 1), (4, 1), (3, 2), (4, 3)])
def test_chain_rule_from_the_sums_matches_autograd(qd):
    from gpytorch_amd.kernels import sm_dense

    q, d = qd
    gen = torch.Generator().manual_seed(17 * q + d)
    x1, x2 = torch.rand(23, d, generator=gen, dtype=torch.float64), torch.rand(19, d, generator=gen, dtype=torch.float64)
    w = (0.3 + torch.rand(q, generator=gen, dtype=torch.float64)).requires_grad_(True)
    mu = (0.5 + 2.5 * torch.rand(q, 1, d, generator=gen, dtype=torch.float64)).requires_grad_(True)
    sigma = (0.9 + 0.5 * torch.rand(q, 1, d, generator=gen, dtype=torch.float64)).requires_grad_(True)
    W = torch.randn(23, 19, generator=gen, dtype=torch.float64)
    gw, gmu, gsg = torch.autograd.grad((W * sm_dense(x1, x2, w, mu, sigma)).sum(), [w, mu, sigma])
    g0, A, B, C = R.sm_sums(x1, x2, w.detach(), mu.detach().reshape(q, d), sigma.detach().reshape(q, d), W)[:4]
    dw, dmu, dsg = R.sm_param_grads(A, B, C, sigma.detach().reshape(q, d))
    for a, b in ((dw, gw), (dmu, gmu.reshape(q, d)), (dsg, gsg.reshape(q, d))):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-11
    assert abs(g0 - float((W * sm_dense(x1, x2, w, mu, sigma)).sum().detach())) < 1e-10 * max(1.0, abs(g0))


def test_normalised_sums_give_the_same_gradients():
    """What ``functions._sm_hyper_grads`` does with the kernel's NORMALISED sums (features carry sqrt(w / Wsum), the outputscale slot Wsum^d), restated
    on the host: the total derivative with respect to w is the outputscale path plus the theta path."""
    q, d = 3, 2
    gen = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(21, d, generator=gen, dtype=torch.float64), torch.rand(17, d, generator=gen, dtype=torch.float64)
    w, mu, sigma = 0.3 + torch.rand(q, generator=gen, dtype=torch.float64), 0.5 + torch.rand(q, d, generator=gen, dtype=torch.float64), 0.9 + torch.rand(q, d, generator=gen, dtype=torch.float64)
    W = torch.randn(21, 17, generator=gen, dtype=torch.float64)
    g0, A, B, C = R.sm_sums(x1, x2, w, mu, sigma, W)[:4]
    ws = w.sum()
    what = w / ws
    s = ws ** d
    g0n, An, Bn, Cn = g0 / s, A * what.reshape(q, 1) / ws ** (d - 1), B / s, C / s        # the kernel's outputs
    d_os = g0n
    d_w = s / ws * (An.sum(1) / what - d * g0n) + d_os * d * ws ** (d - 1)
    rw, rmu, rsg = R.sm_param_grads(A, B, C, sigma)
    assert torch.allclose(d_w, rw, rtol=1e-12) and torch.allclose(-2 * math.pi * s * Cn, rmu, rtol=1e-12)
    assert torch.allclose(-4 * math.pi ** 2 * s * sigma * Bn, rsg, rtol=1e-12)


def test_signed_split_is_exact_toward_zero():
    """K is signed in this family: hi = f16(K) rounded TOWARD ZERO (what v_cvt_pkrtz does on both signs), lo = K - hi -- exact in float32, |lo| below one
    f16 step of hi and of K's sign, so hi + lo restores K to the f16 resolution of lo, as for K >= 0."""
    gen = torch.Generator().manual_seed(0)
    k = (torch.rand(20000, generator=gen) * 2 - 1) * 4096.0            # 2^12 K, K in [-1, 1]
    k = torch.cat([k, -k, torch.tensor([0.0, -0.0, 4096.0, -4096.0, 1e-3, -1e-3])])
    near = k.to(torch.float16).float()
    step = torch.where(near.abs() > k.abs(), torch.nextafter(near.to(torch.float16), torch.zeros_like(near).to(torch.float16)).float(), near)
    hi = step                                                            # round toward zero
    assert bool((hi.abs() <= k.abs()).all())
    lo = k - hi
    assert bool(((lo.double() + hi.double()) == k.double()).all())       # exact difference
    assert bool((torch.sign(lo) * torch.sign(k) >= 0).all())
    lo16 = lo.to(torch.float16).float()
    assert float(((hi + lo16) - k).abs().max() / 4096.0) < 2.0 ** -21


def test_module_surface():
    import gpytorch_amd as g
    from gpytorch_amd.module import Positive

    K = g.kernels.SpectralMixtureKernel
    with pytest.raises(RuntimeError, match="num_mixtures is a required argument"):
        K()
    k = K(num_mixtures=4, ard_num_dims=2)
    assert k.is_stationary and k.num_mixtures == 4 and k.ard_num_dims == 2 and not k.has_lengthscale
    assert k.raw_mixture_weights.shape == (4,) and k.raw_mixture_means.shape == (4, 1, 2) and k.raw_mixture_scales.shape == (4, 1, 2)
    assert {n for n, _ in k.named_parameters()} == {"raw_mixture_weights", "raw_mixture_means", "raw_mixture_scales"}
    for name in ("raw_mixture_weights", "raw_mixture_means", "raw_mixture_scales"):
        assert isinstance(k.constraint_for(name), Positive)
    k.mixture_weights = torch.tensor([0.1, 0.2, 0.3, 0.4])
    k.mixture_means = 1.5
    k.mixture_scales = torch.full((4, 1, 2), 0.7)
    assert torch.allclose(k.mixture_weights, torch.tensor([0.1, 0.2, 0.3, 0.4])) and torch.allclose(k.mixture_means, torch.full((4, 1, 2), 1.5))
    assert torch.allclose(k.mixture_scales, torch.full((4, 1, 2), 0.7))
    kb = K(num_mixtures=3, ard_num_dims=1, batch_shape=torch.Size([2]))
    assert kb.raw_mixture_weights.shape == (2, 3) and kb.raw_mixture_means.shape == (2, 3, 1, 1) and kb.batch_shape == torch.Size([2])
    with pytest.raises(RuntimeError, match="dimensionality"):
        k(torch.rand(5, 3))
    with pytest.raises(RuntimeError, match="SpectralMixtureKernel expected the input to have 2 dimensionality"):
        k.forward(torch.rand(5, 3), torch.rand(5, 3))
    torch.manual_seed(0)
    x, y = torch.rand(40, 2), torch.randn(40)
    k.initialize_from_data(x, y)
    assert k.mixture_means.shape == (4, 1, 2) and k.mixture_scales.shape == (4, 1, 2) and k.mixture_weights.shape == (4,)
    assert bool((k.mixture_means > 0).all()) and bool((k.mixture_scales > 0).all()) and bool((k.mixture_weights > 0).all())
    assert torch.allclose(k.mixture_weights, (y.std() / 4).expand(4), rtol=1e-5)
    with pytest.raises(RuntimeError, match="should be tensors"):
        k.initialize_from_data([0.0], y)
    assert not hasattr(k, "initialize_from_data_empspect")
    assert "SpectralMixtureKernel" in g.kernels.__all__


def test_recognition_rule():
    import gpytorch_amd as g
    from gpytorch_amd import backend as B
    from gpytorch_amd.kernels import sm_native

    K = g.kernels.SpectralMixtureKernel
    table = [  # Q, d, accepted
        (1, 1, True), (8, 1, True), (9, 1, False), (4, 2, True), (5, 2, False), (4, 3, True), (5, 3, False), (1, 4, False)]
    for q, d, ok in table:
        assert B.sm_envelope_ok(q, d) == ok
        assert sm_native(K(q, ard_num_dims=d), torch.rand(6, d)) == ok, (q, d)
    k = K(4)
    assert sm_native(k, torch.rand(6)) and sm_native(k, torch.rand(6, 1), torch.rand(5, 1))
    assert not sm_native(k, torch.rand(6, 1).double())                                  # float64
    assert not sm_native(k, torch.rand(6, 1), torch.rand(5, 1).double())
    assert not sm_native(K(4).double(), torch.rand(6, 1))
    assert not sm_native(k, torch.rand(2, 6, 1))                                        # input batch
    assert not sm_native(K(4, batch_shape=torch.Size([2])), torch.rand(6, 1))           # kernel batch
    assert not sm_native(K(2, ard_num_dims=2), torch.rand(6, 2), last_dim_is_batch=True)
    assert B.KIND_IDS["sm"] == 7


def _set(k, t):
    k.mixture_weights, k.mixture_means, k.mixture_scales = t["w"].to(k.raw_mixture_weights.dtype), t["mu"].to(k.raw_mixture_weights.dtype), t["sigma"].to(k.raw_mixture_weights.dtype)


def test_native_call_builds_one_fused_operator_and_diag_needs_no_launch():
    import gpytorch_amd as g
    from gpytorch_amd.operators import FusedKernelLinearOperator

    t, _, _ = _case("d")
    k = g.kernels.SpectralMixtureKernel(3, ard_num_dims=2)
    _set(k, t)
    x = t["x1"].float()
    op = k(x)
    assert isinstance(op, FusedKernelLinearOperator) and op.spec.kind == "sm" and op.shape == (17, 17)
    ws = float(t["w"].sum())
    assert abs(float(op.outputscale) - ws ** 2) < 1e-5 and op.outputscale.requires_grad and op.spec.param.requires_grad
    assert op.spec.param.numel() == 3 * (1 + 2 * 2) and bool((op.lengthscale == 1).all()) and not op.lengthscale.requires_grad
    assert torch.allclose(k(x, diag=True), torch.full((17,), ws ** 2))                  # equal inputs: Wsum^d, no device
    sc = g.kernels.ScaleKernel(k)
    sc.outputscale = 2.0
    assert isinstance(sc(x), FusedKernelLinearOperator) and abs(float(sc(x).outputscale) - 2.0 * ws ** 2) < 1e-4


def test_declined_calls_take_the_dense_branch_with_reference_values():
    import gpytorch_amd as g
    from gpytorch_amd.operators import DenseLinearOperator, to_dense

    # float64: the golden case itself
    t, _, _ = _case("d")
    k = g.kernels.SpectralMixtureKernel(3, ard_num_dims=2).double()
    _set(k, t)
    out = k(t["x1"], t["x2"])
    assert isinstance(out, DenseLinearOperator)
    assert float((to_dense(out) - t["K"]).abs().max()) < 1e-12
    # diag of two different inputs
    t, diag, _ = _case("g")
    assert diag
    _set(k, t)
    assert float((k(t["x1"], t["x2"], diag=True) - t["K"]).abs().max()) < 1e-12
    k32 = g.kernels.SpectralMixtureKernel(3, ard_num_dims=2)
    _set(k32, t)
    assert float((k32(t["x1"].float(), t["x2"].float(), diag=True).double() - t["K"]).abs().max()) < 1e-5
    # last_dim_is_batch as the reference computes it
    t, _, ldb = _case("h")
    assert ldb
    _set(k, t)
    out = k(t["x1"], t["x2"], last_dim_is_batch=True)
    assert isinstance(out, DenseLinearOperator) and float((to_dense(out) - t["K"]).abs().max()) < 1e-12
    # Q d outside the envelope, float32
    gen = torch.Generator().manual_seed(1)
    k9 = g.kernels.SpectralMixtureKernel(9)
    k9.mixture_weights, k9.mixture_means, k9.mixture_scales = 0.3 + torch.rand(9, generator=gen), 0.5 + torch.rand(9, 1, 1, generator=gen), 0.9 + torch.rand(9, 1, 1, generator=gen)
    x = torch.rand(15, 1, generator=gen)
    out = k9(x)
    assert isinstance(out, DenseLinearOperator)
    ref = R.sm_cov(x, x, k9.mixture_weights.detach(), k9.mixture_means.detach().reshape(9, 1), k9.mixture_scales.detach().reshape(9, 1))
    assert float((to_dense(out).double() - ref).abs().max() / ref.abs().max()) < 1e-5
    # batches
    kb = g.kernels.SpectralMixtureKernel(2, batch_shape=torch.Size([3])).double()
    xb = torch.rand(3, 7, 1, dtype=torch.float64)
    ob = kb(xb)
    assert isinstance(ob, DenseLinearOperator) and to_dense(ob).shape == (3, 7, 7)
    for b in range(3):
        ref = R.sm_cov(xb[b], xb[b], kb.mixture_weights[b].detach(), kb.mixture_means[b].detach().reshape(2, 1), kb.mixture_scales[b].detach().reshape(2, 1))
        assert float((to_dense(ob)[b] - ref).abs().max()) < 1e-12


def test_abi_refusals_before_any_launch():
    from gpytorch_amd import backend as B
    from gpytorch_amd._lib import lib

    h = lib()
    assert h.gpamd_abi_version() == 5
    blk = (torch.zeros(8),)          # any non-null pointer: every refusal below comes before a launch
    p = blk[0].data_ptr()
    args_tail = (None, 300, None, 300)
    # (Q, d) outside the envelope
    for q, d in ((0, 1), (9, 1), (5, 2), (5, 3), (1, 0), (1, 4)):
        assert h.gpamd_kv_sm_partials_f32(p, q, d, *args_tail, d + 2 * q * d, None, 300, 11, None, 300, 1, 384, None, None) == -2
        assert h.gpamd_last_error().startswith(b"kv_sm:") and b"envelope" in h.gpamd_last_error()
        assert h.gpamd_kv_sm_grad_f32(p, q, d, *args_tail, d + 2 * q * d, None, 300, None, 300, 3, None, None, 0, None) == -2
        assert h.gpamd_last_error().startswith(b"kv_sm_grad:") and b"envelope" in h.gpamd_last_error()
        assert h.gpamd_kv_sm_grad_workspace_doubles(300, 300, 3, q, d) == 0
    # a null block
    assert h.gpamd_kv_sm_partials_f32(None, 4, 1, *args_tail, 9, None, 300, 11, None, 300, 1, 384, None, None) == -1 and b"null parameter block" in h.gpamd_last_error()
    assert h.gpamd_kv_sm_grad_f32(None, 4, 1, *args_tail, 9, None, 300, None, 300, 3, None, None, 0, None) == -1 and b"null parameter block" in h.gpamd_last_error()
    # a width that is not d + 2 Q d
    for width in (8, 10, 12):
        assert h.gpamd_kv_sm_partials_f32(p, 4, 1, *args_tail, width, None, 300, 11, None, 300, 1, 384, None, None) == -1 and b"d + 2 Q d" in h.gpamd_last_error()
        assert h.gpamd_kv_sm_grad_f32(p, 4, 1, *args_tail, width, None, 300, None, 300, 3, None, None, 0, None) == -1 and b"d + 2 Q d" in h.gpamd_last_error()
    # the shared checks still apply (bad shape, leading dimensions), and a too-small derivative workspace
    assert h.gpamd_kv_sm_partials_f32(p, 4, 1, None, 0, None, 300, 9, None, 300, 11, None, 300, 1, 384, None, None) == -1
    assert h.gpamd_kv_sm_partials_f32(p, 4, 1, *args_tail, 9, None, 299, 11, None, 300, 1, 384, None, None) == -1
    need = h.gpamd_kv_sm_grad_workspace_doubles(300, 300, 3, 4, 1)
    assert need > 0 and need % (1 + 3 * 4) == 0
    assert h.gpamd_kv_sm_grad_f32(p, 4, 1, p, 300, p, 300, 9, p, 300, p, 300, 3, p, p, need - 1, None) == -3
    # the plan: kind 7 with the prepared width as d, the split flag required; every other entry point refuses the family
    assert h.gpamd_kv_plan(7, 2000, 2000, 9, 11, 0, 2000, None, None, None) == -1 and b"GPAMD_KV_SPLIT" in h.gpamd_last_error()
    for width in (1, 2, 4, 8, 12, 19, 28):
        assert h.gpamd_kv_plan(7, 2000, 2000, width, 11, B.KV_SPLIT, 2000, None, None, None) == -1 and b"prepared width" in h.gpamd_last_error()
    assert h.gpamd_kv_partials_f32(7, 0.0, None, 300, None, 300, 9, None, None, 300, 11, None, 300, 1, 384, B.KV_SPLIT, None, None) == -1
    assert b"parameter block" in h.gpamd_last_error()
    assert h.gpamd_kv_f32(7, 0.0, None, 300, None, 300, 9, None, None, 300, 11, None, None, None, 0, None, 300, None, 1 << 30, B.KV_SPLIT, None) == -1
    assert h.gpamd_prep_points_f32(7, 0.0, None, 10, 1, 1, None, 1, None, None, 4, None) == -1
    assert h.gpamd_kernel_dense_f32(7, 0.0, None, 10, None, 10, 4, None, None, 10, None) == -1
    assert h.gpamd_kv_grad_param_far_f32(7, 0.0, None, 10, None, 10, 4, None, 12, None, 12, 1, 0, None, None, 0, None, None, None, None, None, 0.0, None, 0) == -1


def test_python_refusals():
    from gpytorch_amd import backend as B

    th = torch.rand(4 * 3) + 0.5
    with pytest.raises(ValueError, match="Q \\(1 \\+ 2 d\\)"):
        B.sm_theta_split(torch.rand(7), 1)
    par = B.SMParams(th, 1)
    assert (par.q, par.d, par.width) == (4, 1, 9) and par.block.shape == (4,) and par.block.dtype == torch.float32
    assert torch.allclose(par.block.double(), -2 * math.pi ** 2 * math.log2(math.e) * par.sigma.reshape(-1) ** 2, rtol=1e-6)
    x = torch.rand(10, 1)
    xp = B.sm_prep(x, x.mean(0), par)
    assert xp.shape == (10, 12) and xp.dtype == torch.float32 and bool((xp[:, 9:] == 0).all())
    amp2 = (xp[:, 1:9].reshape(10, 4, 2) ** 2).sum(-1)                       # cos^2 + sin^2 = w^
    assert torch.allclose(amp2.double(), par.what.expand(10, 4), rtol=1e-6)
    P = B.PreparedPoints(xp, 10, 9, 12, "sm", par)
    assert B.far_cull(P, P) is None and B.kv_flags(P, P, 1) == B.KV_SPLIT and B.kv_flags(P, P, 65) == B.KV_SPLIT and not B.grad_gram_ok(P, P)
    k = B.sm_cov(P, P).double() * par.wsum
    ref = R.sm_cov(x, x, par.w, par.mu, par.sigma)
    assert float((k - ref).abs().max() / ref.abs().max()) < 1e-5
    assert float((B.kernel_rows(P, torch.tensor([3, 7]), P).double() * par.wsum - ref[[3, 7]]).abs().max()) < 1e-5
    assert float((B.kernel_diag(P, P) - 1).abs().max()) < 1e-6
