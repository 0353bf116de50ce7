"""The step reference of tests/solver_steps_ref.py, checked WITHOUT a GPU: its steps chained into whole solves must reproduce the oracles
(oracle/linear_cg.py, oracle/lanczos.py) and dense linear algebra.  This is what entitles the reference to judge the kernels one step
at a time in tests/test_gpu_solver_steps.py."""
import math

import pytest
import torch

from gpytorch_amd.linear_cg import build_tridiag
from oracle import lanczos as OL
from oracle import linear_cg as OCG
from oracle.pivoted_cholesky import build_preconditioner
from tests import solver_steps_ref as S

F64 = torch.float64
RTOL = 1e-10


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _system(n=300, rank=10, sigma2=0.5, seed=0):
    g = torch.Generator().manual_seed(seed)
    Lf = 0.2 * torch.randn(n, rank, generator=g, dtype=F64)   # (lambda_max ~ 15: the un-preconditioned solve converges too)
    G = torch.randn(n, n, generator=g, dtype=F64)
    A = Lf @ Lf.t() + sigma2 * torch.eye(n, dtype=F64) + 0.1 * (G @ G.t()) / n
    rhs = torch.randn(n, 4, generator=g, dtype=F64)
    rhs[:, 2] = 0.0   # one zero right-hand side
    return A, Lf, sigma2, rhs


@pytest.mark.parametrize("precond", [False, True])
def test_cg_steps_chain_equals_oracle(precond):
    n, t, max_iter, max_tri, tol = 300, 4, 200, 20, 1e-4   # (d.q < eps = 1e-10 masks alpha once |r| ~ 1e-5: no tighter tolerance is reachable)
    A, Lf, sigma2, rhs = _system(n)
    pre = build_preconditioner(Lf, sigma2)[0] if precond else None
    Xo, To, info = OCG.linear_cg(lambda V: A @ V, rhs, n_tridiag=t, tolerance=tol, max_iter=max_iter, max_tridiag_iter=max_tri, preconditioner=pre,
                                 return_info=True)
    assert info["tolerance_reached"]

    n_tri_iter = min(max_tri, n)
    hist = min(n_tri_iter, max_iter)
    st = S.CgRef(n, t, hist_len=hist, precond=precond)
    S.cg_init(st, rhs.t().contiguous(), 1 if precond else 0)
    if precond:
        st.Z = pre(st.R.t()).t().contiguous()
        st.D = st.Z.clone()
        S.cg_begin(st)
    min_iter, floor = min(10, max_iter - 1), min(n_tri_iter, max_iter - 1)
    for k in range(max_iter):
        S.cg_reduce_q(st, (A @ st.D.t()).t().unsqueeze(0))
        S.cg_update_xr(st, k)
        if precond:
            st.Z = pre(st.R.t()).t().contiguous()
        S.cg_update_d(st, k)
        S.cg_stop(st, k, min_iter, floor, tol)
        if st.done[0]:
            break
    S.cg_finish(st)

    assert st.done == [1, info["iters"]]
    assert rel(st.X.t(), Xo) < RTOL
    assert bool((st.X[2] == 0).all()) and float(st.rnorm[2]) == 0.0 and bool(st.zero_rhs[2])
    rows = min(hist, info["iters"])
    assert rel(st.alpha_hist[:rows], torch.stack(info["alpha"][:rows])) < RTOL
    assert rel(st.beta_hist[:rows], torch.stack(info["beta"][:rows])) < RTOL
    T = build_tridiag(st.alpha_hist, st.beta_hist, st.done[1], True, n_tri_iter)
    assert T.shape == To.shape and rel(T, To) < RTOL
    assert rel(st.rnorm, info["rnorm"]) < 1e-6   # (|r| near the tolerance: a difference of rounding errors)


def test_lanczos_steps_chain_equals_oracle():
    """The driver of gpytorch_amd/lanczos.py (lanczos_steps) restated on the reference steps."""
    n, num_iter, tol = 120, 25, 1e-5
    A = _system(n, seed=1)[0]
    g = torch.Generator().manual_seed(2)
    init = torch.randn(n, 1, generator=g, dtype=F64)
    Qo, To = OL.lanczos_tridiag(lambda V: A @ V, num_iter, n, init, tol=tol)

    Q = torch.zeros(num_iter, n, dtype=F64)
    alpha, beta = torch.zeros(num_iter, dtype=F64), torch.zeros(num_iter, dtype=F64)

    def project(basis, r, tol_=-1.0, flag=0):
        return S.lanczos_coef(S.lanczos_project(basis, r).unsqueeze(1), tol_, flag)   # one finished partial per coefficient

    r, rr = S.lanczos_subtract(Q[0:1], torch.zeros(1, dtype=F64), init.reshape(-1))
    Q[0] = S.lanczos_normalize(r, rr, 1e-6, 0)[0]
    r = S.lanczos_residual(A @ Q[0])
    alpha[0:1] = project(Q[0:1], r)[0]
    r, rr = S.lanczos_subtract(Q[0:1], alpha[0:1], r)
    Q[1], b, _ = S.lanczos_normalize(r, rr, 1e-6, 0)
    beta[0] = b
    m = 2
    for k in range(1, num_iter):
        r = S.lanczos_residual(A @ Q[k], Q[k - 1], beta[k - 1])
        alpha[k:k + 1] = project(Q[k:k + 1], r)[0]
        m = k + 1
        if k + 1 >= num_iter:
            break
        r, rr = S.lanczos_subtract(Q[k:k + 1], alpha[k:k + 1], r)
        r, rr = S.lanczos_subtract(Q[:k + 1], project(Q[:k + 1], r)[0], r)
        r, b, stop = S.lanczos_normalize(r, rr, 1e-6, 0)
        beta[k] = b
        ok = False
        for _ in range(10):
            coef, need = project(Q[:k + 1], r, tol, 0)
            if not need:
                ok = True
                break
            r, rr = S.lanczos_subtract(Q[:k + 1], coef, r)
            r = S.lanczos_normalize(r, rr, 1e-6, 0)[0]
        Q[k + 1] = r
        if stop or not ok:
            break
        m = k + 2
    T = torch.diag(alpha[:m]) + torch.diag(beta[:m - 1], 1) + torch.diag(beta[:m - 1], -1)
    assert T.shape == To.shape and rel(T, To) < RTOL
    assert rel(Q[:m].t(), Qo) < 1e-9   # (the oracle groups the re-orthogonalisation sums differently: rounding only)


def test_lanczos_step_flags():
    part = torch.tensor([[1e-6, 2e-6], [-3e-3, 1e-3]], dtype=F64)
    assert S.lanczos_coef(part, 1e-2, 0)[1] == 0 and S.lanczos_coef(part, 1e-3, 0)[1] == 1
    assert S.lanczos_coef(part, 1e-2, 1)[1] == 1 and S.lanczos_coef(part, -1.0, 0)[1] == 0
    r = torch.ones(3, dtype=F64)
    out, nrm, stop = S.lanczos_normalize(r, 0.0, 1e-6, 0)
    assert bool((out == 0).all()) and nrm == 0.0 and stop == 1
    assert S.lanczos_normalize(r, -1e-20, 1e-6, 0)[1:] == (0.0, 1)
    assert S.lanczos_normalize(r, 4e-12, 1e-6, 0)[2] == 0


def test_precond_steps_equal_dense_solve():
    n, k, sigma2 = 300, 10, 0.5
    _, Lf, _, rhs = _system(n, k, sigma2)
    Q1 = build_preconditioner(Lf, sigma2)[2]
    R = rhs.t().contiguous()
    W = S.precond_coef(R, Q1.t())
    out = S.precond_apply(R, Q1.t(), W, sigma2)
    ref = torch.linalg.solve(Lf @ Lf.t() + sigma2 * torch.eye(n, dtype=F64), rhs).t()
    assert rel(out, ref) < RTOL


def test_block_and_minres_steps():
    g = torch.Generator().manual_seed(3)
    n, k, b = 50, 7, 3
    Q = torch.linalg.qr(torch.randn(n, k, generator=g, dtype=F64))[0].t().contiguous()
    R = torch.randn(b, n, generator=g, dtype=F64)
    W = S.block_project(R, Q)
    R1 = S.block_subtract(Q, W, R)
    assert float((R1 @ Q.t()).abs().max()) < 1e-13          # orthogonal to the basis afterwards
    M = torch.linalg.inv(torch.linalg.cholesky(R1 @ R1.t()))   # Cholesky-QR: lower triangular, NOT symmetric
    R2 = S.block_transform(M, R1)
    assert rel(R2 @ R2.t(), torch.eye(b, dtype=F64)) < 1e-12
    # one MINRES direction update against the formula written out per element
    v, d1, d2, x = (torch.randn(*s, generator=g, dtype=F64) for s in ((2, n), (3, 2, n), (3, 2, n), (3, 2, n)))
    coef = torch.randn(4, 3, 2, generator=g, dtype=F64)
    d, xn = S.msminres_update(v, d1, d2, x, coef)
    q, c, i = 2, 1, 17
    dd = (v[c, i] - coef[0, q, c] * d1[q, c, i] - coef[1, q, c] * d2[q, c, i]) * coef[2, q, c]
    assert math.isclose(float(d[q, c, i]), float(dd), rel_tol=1e-14)
    assert math.isclose(float(xn[q, c, i]), float(x[q, c, i] + coef[3, q, c] * dd), rel_tol=1e-14)


def test_kv_reduce_and_stop_rule():
    g = torch.Generator().manual_seed(4)
    P, Vd, dv = torch.randn(3, 2, 9, generator=g, dtype=F64), torch.randn(2, 9, generator=g, dtype=F64), torch.rand(9, generator=g, dtype=F64)
    assert rel(S.kv_reduce(P, 2.0, 0.5, dv, Vd), 2.0 * P.sum(0) + (0.5 + dv) * Vd) < 1e-15
    assert rel(S.kv_reduce(P, None, 0.5, dv, None), P.sum(0)) < 1e-15
    st = S.CgRef(5, 2)
    for k, mean, want in ((10, 0.5, [1, 11]), (9, 0.5, [0, 10]), (10, 1.0, [0, 11]), (10, float("nan"), [2, 11])):
        st.done = [0, 0]
        st.stats[:2] = torch.tensor([2 * mean, 2.0], dtype=F64)
        S.cg_stop(st, k, 10, 0, 1.0)
        assert st.done == want
    st.done = [0, 0]
    st.stats[:2] = torch.tensor([0.0, 2.0], dtype=F64)
    S.cg_stop(st, 10, 10, 11, 1.0)
    assert st.done == [0, 11]
