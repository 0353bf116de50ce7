"""CPU: ``DistributionalInputKernel`` / ``GaussianSymmetrizedKLKernel`` without a GPU -- the dense branch against the float64 restatement
(tests/skl_ref.py) and against values produced by executing the reference's own ``_symmetrized_kl`` / ``forward`` (tests/golden/skl_values.npz), the
closed-form derivatives of the restatement against central differences, the prepared rows, the ``skl_native`` rule, the state dict."""
import collections
import os

import numpy as np
import pytest
import torch

import gpytorch_amd as g
from gpytorch_amd import families as F
from gpytorch_amd import kernels as KK
from gpytorch_amd.operators import DenseLinearOperator, to_dense
from tests.skl_ref import central_difference, skl_grad_sums, skl_K, skl_S
from tests.util import rel_err

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "skl_values.npz"))
CASES = sorted({k.split("_")[0] for k in GOLD.files})


@pytest.mark.parametrize("name", CASES)
def test_dense_and_restatement_match_the_reference_values(name):
    d, f64 = int(name[1]), name.endswith("64")
    x1 = torch.from_numpy(GOLD[f"{name}_x1"])
    x2 = torch.from_numpy(GOLD[f"{name}_x2"]) if f"{name}_x2" in GOLD.files else x1
    S, K, dg = (torch.from_numpy(GOLD[f"{name}_{k}"]) for k in ("S", "K", "diag_pair"))
    tol = 1e-12 if f64 else 2e-5
    assert len(CASES) == 16 and K.shape == (x1.shape[0], x2.shape[0])
    assert rel_err(skl_S(x1.double(), x2.double()), S) < tol and rel_err(skl_K(x1.double(), x2.double(), float(d)), K) < tol
    ls = torch.tensor([[float(d)]], dtype=x1.dtype)
    k = dg.shape[0]
    assert rel_err(KK.skl_dense(x1, x2, ls), K) < tol and rel_err(KK.skl_dense(x1[:k], x2[:k], ls, diag=True), dg) < tol
    ker = g.kernels.GaussianSymmetrizedKLKernel().to(x1.dtype)
    ker.lengthscale = float(d)
    op = ker(x1, x2)
    assert isinstance(op, DenseLinearOperator) and rel_err(to_dense(op), K) < tol
    assert rel_err(ker(x1[:k], x2[:k], diag=True), dg) < tol


@pytest.mark.parametrize("d", [1, 3])
def test_closed_form_derivatives_match_central_differences(d):
    gen = torch.Generator().manual_seed(d)
    X1, X2 = (torch.cat([torch.rand(n, d, generator=gen, dtype=torch.float64), -3 + 2 * torch.rand(n, d, generator=gen, dtype=torch.float64)], -1) for n in (5, 4))
    W, ls = torch.randn(5, 4, generator=gen, dtype=torch.float64), float(d)
    g0, g1, g_mu, g_a = skl_grad_sums(X1, X2, ls, W)
    num = central_difference(lambda x: (W * skl_K(x, X2, ls)).sum(), X1)
    assert rel_err(g_mu, num[:, :d]) < 1e-7 and rel_err(g_a * X1[:, d:].exp(), num[:, d:]) < 1e-7       # da / d(log sigma^2) = exp(log sigma^2)
    num_l = central_difference(lambda l: (W * skl_K(X1, X2, l)).sum(), torch.tensor(ls, dtype=torch.float64))
    assert abs(float(g1) / (2 * ls * ls) - float(num_l)) < 1e-7 * abs(float(num_l)) and rel_err(g0, (W * skl_K(X1, X2, ls)).sum()) < 1e-14


@pytest.mark.parametrize("d,db,width", [(1, 1, 4), (2, 4, 12), (4, 4, 12), (5, 6, 20), (6, 6, 20)])
def test_prepared_rows_and_pointwise_covariance(d, db, width):
    """[mu - shift | a | b] in blocks of DB columns, zero padding in every block; ``skl_cov`` on them is the restatement, with an exact unit diagonal."""
    gen = torch.Generator().manual_seed(d)
    x = torch.cat([torch.rand(9, d, generator=gen), -3 + 2 * torch.rand(9, d, generator=gen)], -1)
    shift = x[:, :d].mean(0)
    rows, dvar = F.skl_prep(x, shift)
    assert (F.skl_block(d), F.skl_width(d)) == (db, width) and rows.shape == (9, width) and rows.dtype == torch.float32 and dvar.dtype == torch.float64
    a = 1e-8 + x[:, d:].double().exp()
    want = torch.zeros(9, width, dtype=torch.float64)
    want[:, :d], want[:, db : db + d], want[:, 2 * db : 2 * db + d] = x[:, :d].double() - shift.double(), a, 1 / a
    assert torch.equal(rows, want.float())
    P = collections.namedtuple("P", "xp n param")
    p = P(rows, 9, F.SKLParams(d, torch.tensor([[float(d)]]), dvar))
    K = F.skl_cov(p, p)
    assert rel_err(K, skl_K(x.double(), x.double(), float(d))) < 1e-5 and torch.equal(K.diagonal(), torch.ones(9))
    for bad in (torch.tensor([1.0, 2.0]), torch.tensor([0.0]), torch.tensor([float("inf")])):
        with pytest.raises(ValueError):
            F.SKLParams(d, bad, dvar)


def test_entry_points_refuse_before_any_launch():
    """GPAMD_EUNSUPPORTED (-2) for a width outside 4 / 12 / 20, GPAMD_EINVAL (-1) for a bad lengthscale, null pointers or kind 13 without its flag,
    GPAMD_EWORKSPACE (-3) for a short workspace; the plan accepts the three widths under kind 13."""
    import ctypes as C

    from gpytorch_amd._lib import lib

    L, p = lib(), C.c_void_p(64)   # (a non-null address that is never read: every call below returns before a launch)
    assert [int(L.gpamd_kv_skl_grad_workspace_doubles(300, 200, 5, w)) > 0 for w in (4, 8, 12, 16, 20)] == [True, False, True, False, True]
    need = int(L.gpamd_kv_skl_grad_workspace_doubles(300, 200, 5, 12))
    call = lambda ls, w, x, ws: L.gpamd_kv_skl_grad_f32(ls, x, 300, p, 200, w, p, 300, p, 200, 5, p, p, ws, None)  # noqa: E731
    assert call(2.0, 8, p, need) == -2 and call(0.0, 12, p, need) == -1 and call(float("nan"), 12, p, need) == -1
    assert call(2.0, 12, None, need) == -1 and call(2.0, 12, p, need - 1) == -3
    S, jc, ws = C.c_int(0), C.c_int(0), C.c_int64(0)
    for w, rc in ((4, 0), (12, 0), (20, 0), (8, -1)):
        assert L.gpamd_kv_plan(F.SKL_KIND_ID, 5000, 4000, w, 11, 8, 5000, C.byref(S), C.byref(jc), C.byref(ws)) == rc
    assert L.gpamd_kv_plan(F.SKL_KIND_ID, 5000, 4000, 12, 11, 0, 5000, C.byref(S), C.byref(jc), C.byref(ws)) == -1
    assert L.gpamd_kv_partials_f32(F.SKL_KIND_ID, 0.0, p, 300, p, 200, 12, None, p, 200, 5, p, 300, 1, 256, 8, None, None) == -1


def test_native_rule_state_dict_and_user_distance():
    """``skl_native`` case by case on stand-ins that carry what the rule reads (it never touches values); the reference's parameter names; exports;
    ``DistributionalInputKernel`` with a distance function of the user's."""
    T = collections.namedtuple("T", "shape dtype device")
    T.dim = lambda self: len(self.shape)

    def t(*shape, dtype=torch.float32, device="cuda"):
        return T(torch.Size(shape), dtype, torch.device(device))

    ker = g.kernels.GaussianSymmetrizedKLKernel()
    for d in range(1, 7):
        assert KK.skl_native(ker, t(30, 2 * d)) and KK.skl_native(ker, t(30, 2 * d), t(7, 2 * d))
    assert not KK.skl_native(ker, t(30, 14)) and not KK.skl_native(ker, t(30, 3)) and not KK.skl_native(ker, t(30, 4), t(7, 6))
    assert not KK.skl_native(ker, t(30, 4, dtype=torch.float64)) and not KK.skl_native(ker, t(30, 4, device="cpu"))
    assert not KK.skl_native(ker, t(2, 30, 4)) and not KK.skl_native(ker, t(30, 4), last_dim_is_batch=True)
    assert not KK.skl_native(g.kernels.GaussianSymmetrizedKLKernel(ard_num_dims=4), t(30, 4))
    assert not KK.skl_native(g.kernels.GaussianSymmetrizedKLKernel(active_dims=[0, 1]), t(30, 2))
    assert not KK.skl_native(g.kernels.GaussianSymmetrizedKLKernel(batch_shape=torch.Size([2])), t(30, 4))
    assert not KK.skl_native(g.kernels.GaussianSymmetrizedKLKernel().double(), t(30, 4))
    assert sorted(ker.state_dict()) == ["raw_lengthscale", "raw_lengthscale_constraint.lower_bound", "raw_lengthscale_constraint.upper_bound"]
    assert ker.has_lengthscale and ker.raw_lengthscale.shape == (1, 1) and issubclass(type(ker), g.kernels.DistributionalInputKernel)
    assert {"DistributionalInputKernel", "GaussianSymmetrizedKLKernel", "skl_native", "skl_dense"} <= set(KK.__all__)
    assert F.SKL_KIND_ID == 13 and F.FAMILIES["skl"].id == 13 and "skl" not in F.KIND_IDS
    with pytest.raises(NotImplementedError):
        g.kernels.DistributionalInputKernel(None)
    x1, x2 = torch.rand(6, 3, dtype=torch.float64), torch.rand(4, 3, dtype=torch.float64)
    mine = g.kernels.DistributionalInputKernel(lambda a, b: (a.unsqueeze(-2) - b.unsqueeze(-3)).abs().sum(-1)).double()
    mine.lengthscale = 0.7
    ref = torch.exp(-torch.cdist(x1, x2, p=1) / 0.7)
    assert rel_err(to_dense(mine(x1, x2)), ref) < 1e-12 and rel_err(mine(x1[:4], x2, diag=True), ref[:4].diagonal()) < 1e-12
