"""Float64 reference of the solvers' step kernels (mBCG, Lanczos, block Lanczos, preconditioner apply, multi-shift MINRES): one plain
torch function on the CPU per entry point of the C ABI, written from the formulas in ``include/gpamd.h`` and the comments of
``csrc/cg_kernels.hpp`` / ``csrc/lanczos_kernels.hpp``, and from the algorithms of ``oracle/linear_cg.py`` and ``oracle/lanczos.py``.

Every function takes the kernel's float32 / float64 inputs upcast exactly (``.double()``) and returns every output the kernel writes.
Reductions are returned as FINISHED sums (the kernels leave per-workgroup partials that their consumer sums; a test sums the
partials in float64 and compares).  Vectors are probe-major ``[t, n]`` as in the library, WITHOUT padding.

``tests/test_solver_steps_ref_cpu.py`` chains these steps into whole solves and checks them against the oracles: that is what entitles
them to judge the kernels in ``tests/test_gpu_solver_steps.py``.  :class:`CgDevice` (at the end) is the device-side twin of the mBCG
state: a solver handle allocated the way ``gpytorch_amd/linear_cg.py`` does, with the scratch pieces exposed through the documented
layout queries only.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------ generic reductions
def coldot(A, B):
    """gpamd_coldot: out[c] = sum_i A[c][i] B[c][i]."""
    return (A.double() * B.double()).sum(1)


def kv_reduce(P, scale=None, dscale=None, dvec=None, Vd=None):
    """gpamd_kv_reduce: Out = scale * sum_s P[s] + (dscale + dvec) .* Vd.  P [S, t, n]; scale / dscale: python floats or None (= 1 / 0);
    dvec [n] or None; Vd [t, n] or None (then no diagonal term at all, whatever dscale and dvec are)."""
    out = P.double().sum(0) * (1.0 if scale is None else float(scale))
    if Vd is not None:
        diag = torch.full((P.shape[-1],), 0.0 if dscale is None else float(dscale), dtype=F64)
        if dvec is not None:
            diag = diag + dvec.double()
        out = out + diag * Vd.double()
    return out


# ------------------------------------------------------------------------------------------------------------------------- mBCG
class CgRef:
    """The state of one t-column solve (cg_kernels.hpp ``CgState``) in float64.  ``dq`` / ``rz`` / ``rr`` are the finished sums of the three
    partial arrays (d.q -- and |b|^2 during init --, r.z, r.r).  ``Z is R`` without a preconditioner."""

    def __init__(self, n, t, hist_len=0, eps=1e-10, stop_updating_after=1e-10, precond=False):
        self.n, self.t, self.hist_len, self.eps, self.stop_after = n, t, hist_len, float(eps), float(stop_updating_after)
        z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
        self.X, self.R, self.D, self.Q = z(t, n), z(t, n), z(t, n), z(t, n)
        self.Z = z(t, n) if precond else self.R
        self.bnorm, self.rnorm, self.rho, self.stats = z(t), z(t), z(2, t), z(4)
        self.dq, self.rz, self.rr = z(t), z(t), z(t)
        self.alpha_hist, self.beta_hist = z(hist_len, t), z(hist_len, t)
        self.zero_rhs = torch.zeros(t, dtype=torch.bool)
        self.converged = torch.zeros(t, dtype=torch.bool)
        self.done = [0, 0]

    @property
    def same_z(self):
        return self.Z is self.R

    def set_R(self, R):
        """assign R keeping the Z == R aliasing of the un-preconditioned form"""
        same = self.same_z
        self.R = R
        if same:
            self.Z = R


def cg_init_norms(st: CgRef, B):
    """|b_c|^2 (into the d.q partials); clears the done words."""
    st.done = [0, 0]
    st.dq = coldot(B, B)


def cg_init_apply(st: CgRef, B, copy_d):
    """bnorm = |b| (1 for a zero column: |b| < eps); R = B / bnorm; X = 0; D = R when copy_d; r.r (and r.z = r.r when copy_d)."""
    bn = st.dq.sqrt()
    st.zero_rhs = bn < st.eps
    st.bnorm = torch.where(st.zero_rhs, torch.ones_like(bn), bn)
    st.set_R(B.double() / st.bnorm.unsqueeze(1))
    st.X = torch.zeros_like(st.R)
    st.rr = (st.R * st.R).sum(1)
    if copy_d:
        st.D = st.R.clone()
        st.rz = st.rr.clone()


def cg_begin_apply(st: CgRef):
    """rho[0] = r.z; rnorm = |r|; converged = rnorm < stop_updating_after; done = {0, 0}."""
    st.rho[0] = st.rz
    st.rnorm = st.rr.sqrt()
    st.converged = st.rnorm < st.stop_after
    st.done = [0, 0]


def cg_dot_rz(st: CgRef, use_done=True):
    if use_done and st.done[0]:
        return
    st.rz = (st.R * st.Z).sum(1)


def cg_init(st: CgRef, B, have_precond):
    """gpamd_cg_init: norms + apply (+ begin when there is no preconditioner)."""
    cg_init_norms(st, B)
    cg_init_apply(st, B, 0 if have_precond else 1)
    if not have_precond:
        cg_begin_apply(st)


def cg_begin(st: CgRef):
    """gpamd_cg_begin (after the caller wrote Z = P^-1 R and D = Z): rho = r.z."""
    cg_dot_rz(st, use_done=False)
    cg_begin_apply(st)


def cg_reduce_q(st: CgRef, P, scale=None, dscale=None, dvec=None):
    """Q = scale * sum_s P[s] + (dscale + dvec) .* D;  d.q."""
    if st.done[0]:
        return
    st.Q = kv_reduce(P, scale, dscale, dvec, st.D)
    st.dq = (st.D * st.Q).sum(1)


def _iter_index(st: CgRef, k):
    return st.done[1] if k < 0 else k   # k = -1: the count cg_stop maintains


def cg_update_xr(st: CgRef, k):
    """alpha = rho / d.q, 0 where d.q < eps or the column has converged; X += alpha D; R -= alpha Q; r.r (= r.z when Z == R);
    alpha_hist[k] = alpha for k < hist_len."""
    if st.done[0]:
        return
    k = _iter_index(st, k)
    bad = st.dq < st.eps
    alpha = st.rho[k & 1] / torch.where(bad, torch.ones_like(st.dq), st.dq)
    alpha = torch.where(bad | st.converged, torch.zeros_like(alpha), alpha)
    st.set_R(st.R - alpha.unsqueeze(1) * st.Q)
    st.X = st.X + alpha.unsqueeze(1) * st.D
    st.rr = (st.R * st.R).sum(1)
    if st.same_z:
        st.rz = st.rr.clone()
    st.alpha = alpha   # (kept for the tests: the history has a row for k < hist_len only)
    if k < st.hist_len:
        st.alpha_hist[k] = alpha


def cg_update_d_apply(st: CgRef, k):
    """beta = rho_new / rho_old, 0 where rho_old < eps; D = Z + beta D; rho_new into the other half of rho; rnorm = |r| (0 for a zero
    right-hand side); converged; beta_hist[k]; stats = {sum_c rnorm, t}."""
    if st.done[0]:
        return
    k = _iter_index(st, k)
    rho_old = st.rho[k & 1]
    bad = rho_old < st.eps
    beta = st.rz / torch.where(bad, torch.ones_like(rho_old), rho_old)
    beta = torch.where(bad, torch.zeros_like(beta), beta)
    st.D = st.Z + beta.unsqueeze(1) * st.D
    st.rho[(k + 1) & 1] = st.rz
    st.rnorm = torch.where(st.zero_rhs, torch.zeros_like(st.rr), st.rr.sqrt())
    st.converged = st.rnorm < st.stop_after
    st.beta = beta
    if k < st.hist_len:
        st.beta_hist[k] = beta
    st.stats[0] = st.rnorm.sum()
    st.stats[1] = float(st.t)


def cg_update_d(st: CgRef, k):
    if not st.same_z:
        cg_dot_rz(st)
    cg_update_d_apply(st, k)


def cg_stop(st: CgRef, k, min_iter, tridiag_floor, tol):
    """done[1] = k + 1; done[0] = 1 when k >= min_iter and mean < tol and not k < tridiag_floor; a NaN mean: done = {2, k + 1}."""
    if st.done[0]:
        return
    k = _iter_index(st, k)
    mean = float(st.stats[0]) / float(st.stats[1]) if float(st.stats[1]) != 0.0 else math.nan
    st.done[1] = k + 1
    if mean != mean:
        st.done[0] = 2
    elif k >= min_iter and mean < tol and not k < tridiag_floor:
        st.done[0] = 1


def cg_finish(st: CgRef):
    st.X = st.X * st.bnorm.unsqueeze(1)


# ---------------------------------------------------------------------------------------------------------------------- Lanczos
def lanczos_residual(w, q_prev=None, beta_prev=None):
    """r = w - beta_prev q_prev (q_prev None: r = w)."""
    r = w.double().clone()
    if q_prev is not None:
        r = r - (0.0 if beta_prev is None else float(beta_prev)) * q_prev.double()
    return r


def lanczos_project(Q, r):
    """c[m] = <Q[m], r> (project leaves partials, coef finishes them)."""
    return Q.double() @ r.double()


def lanczos_coef(part, tol, flag):
    """coef[m] = sum_b part[m][b]; tol >= 0: flag |= any |coef| > tol.  part [k, nb]; returns (coef, flag)."""
    coef = part.double().sum(1)
    if tol >= 0 and bool((coef.abs() > tol).any()):
        flag = flag | 1
    return coef, flag


def lanczos_subtract(Q, coef, r):
    """r -= sum_m coef[m] Q[m]; returns (r, |r|^2)."""
    out = r.double() - coef.double() @ Q.double()
    return out, float((out * out).sum())


def lanczos_normalize(r, rr, tiny, stop):
    """norm = sqrt(max(rr, 0)); out = r / norm (exact zeros for norm = 0); stop |= norm < tiny.  Returns (out, norm, stop)."""
    nrm = math.sqrt(max(float(rr), 0.0))
    out = r.double() / nrm if nrm > 0 else torch.zeros_like(r.double())
    return out, nrm, (stop | 1) if nrm < tiny else stop


# --------------------------------------------------------------------------------------------- preconditioner / block Lanczos / MINRES
def precond_coef(R, Q1):
    """W[c][m] = sum_i R[c][i] Q1[m][i]   (also block_project with R the block and Q1 the basis)."""
    return R.double() @ Q1.double().t()


block_project = precond_coef


def precond_apply(R, Q1, W, sigma2):
    """Out = (R - W Q1) / sigma2."""
    return (R.double() - W.double() @ Q1.double()) / float(sigma2)


def block_subtract(Q, W, R):
    """R[c] -= sum_m W[c][m] Q[m]."""
    return R.double() - W.double() @ Q.double()


def block_transform(M, R):
    """R[r] = sum_c M[r][c] R[c]."""
    return M.double() @ R.double()


def msminres_update(v, d1, d2, x, coef):
    """d = (v_c - delta d1 - eps d2) / gamma (written over d2); x += tau d.  v [t, n]; d1, d2, x [Q, t, n]; coef [4, Q, t] = delta | eps |
    1 / gamma | tau.  Returns (d, x)."""
    delta, eps, ginv, tau = (coef[j].double().unsqueeze(-1) for j in range(4))
    d = (v.double().unsqueeze(0) - delta * d1.double() - eps * d2.double()) * ginv
    return d, x.double() + tau * d


# ---------------------------------------------------------------------------------------------------------- the device-side twin
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class CgDevice:
    """A solver handle allocated the way gpytorch_amd/linear_cg.py allocates it (X, R, D, Q, Z [t, ld]; fscratch; iscratch), with the
    scratch pieces as views: bnorm / rnorm / alpha_hist / beta_hist / stats by ``gpamd_cg_layout``, rho as the 2 t elements between
    rnorm and stats (include/gpamd.h), the three partial arrays [t, stride] by ``gpamd_cg_partials_layout`` and zero_rhs / converged /
    done by the iscratch layout [zero_rhs(t) | converged(t) | done(2)].  ``fill``: what the vectors (pads included) and the float scratch
    start as."""

    def __init__(self, n, t, ld, dtype, dev, hist_len=0, eps=1e-10, stop_updating_after=1e-10, precond=False, fill=float("nan")):
        from gpytorch_amd._lib import lib

        L = self.L = lib()
        self.n, self.t, self.ld, self.dtype, self.hist_len = n, t, ld, dtype, hist_len
        self.f64 = dtype == torch.float64
        mk = lambda: torch.full((t, ld), fill, device=dev, dtype=dtype)  # noqa: E731
        self.X, self.R, self.D, self.Q = mk(), mk(), mk(), mk()
        self.Z = mk() if precond else self.R
        nf = int((L.gpamd_cg64_fscratch_elems if self.f64 else L.gpamd_cg_fscratch_elems)(t, hist_len))
        self.fs = torch.full((nf,), fill, device=dev, dtype=dtype)
        self.isc = torch.zeros(int(L.gpamd_cg_iscratch_elems(t)), device=dev, dtype=torch.int32)
        o = (C.c_int64 * 5)()
        assert L.gpamd_cg_layout(t, hist_len, o) == 0
        fs = self.fs
        self.bnorm, self.rnorm = fs[o[0]:o[0] + t], fs[o[1]:o[1] + t]
        assert o[4] - (o[1] + t) == 2 * t, "rho [2][t] is documented to lie between rnorm and stats"
        self.rho = fs[o[1] + t:o[4]].view(2, t)
        self.alpha_hist = fs[o[2]:o[2] + hist_len * t].view(hist_len, t)
        self.beta_hist = fs[o[3]:o[3] + hist_len * t].view(hist_len, t)
        self.stats = fs[o[4]:o[4] + 4]
        po, stride, nb = (C.c_int64 * 3)(), C.c_int(), C.c_int()
        assert L.gpamd_cg_partials_layout(n, t, hist_len, po, C.byref(stride), C.byref(nb)) == 0
        self.stride, self.nb = stride.value, nb.value
        self.part_a, self.part_rz, self.part_rr = (fs[po[j]:po[j] + t * self.stride].view(t, self.stride) for j in range(3))
        self.zero_rhs, self.converged, self.done = self.isc[:t], self.isc[t:2 * t], self.isc[2 * t:2 * t + 2]
        create = L.gpamd_cg64_create if self.f64 else L.gpamd_cg_create_f32
        self.h = create(n, t, ld, _ptr(self.X), _ptr(self.R), _ptr(self.D), _ptr(self.Q), _ptr(self.Z), _ptr(self.fs), _ptr(self.isc), hist_len,
                        float(eps), float(stop_updating_after))
        assert self.h, L.gpamd_last_error()

    def fn(self, step):
        """the entry point of a step for this handle's scalar type (float64: the cg64 twins)"""
        return getattr(self.L, f"gpamd_cg64_{step}" if self.f64 else f"gpamd_cg_{step}_f32")

    def close(self):
        if self.h:
            (self.L.gpamd_cg64_destroy if self.f64 else self.L.gpamd_cg_destroy)(self.h)
            self.h = None

    def __del__(self):
        self.close()
