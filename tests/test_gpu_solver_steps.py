"""The solvers' step kernels, ONE STEP PER CASE, from a preset state, through the C ABI (``gpytorch_amd._lib.lib()``) only -- no K*V here: the
products a step consumes are synthetic partial slabs.  Reference: tests/solver_steps_ref.py (float64, checked against the oracles in
tests/test_solver_steps_ref_cpu.py).

Entry points exercised:
  gpamd_coldot_f32 gpamd_coldot_f64 gpamd_kv_reduce_f32 gpamd_kv_reduce_f64
  gpamd_cg_init_f32 gpamd_cg_init_norms_f32 gpamd_cg_init_apply_f32 gpamd_cg_begin_apply_f32 gpamd_cg_begin_f32 gpamd_cg_dot_rz_f32
  gpamd_cg_reduce_q_f32 gpamd_cg_update_xr_f32 gpamd_cg_update_d_f32 gpamd_cg_update_d_apply_f32 gpamd_cg_stop_f32 gpamd_cg_finish_f32
  gpamd_cg64_init gpamd_cg64_begin gpamd_cg64_reduce_q gpamd_cg64_update_xr gpamd_cg64_update_d gpamd_cg64_stop gpamd_cg64_finish
  gpamd_lanczos_residual_f32 gpamd_lanczos_project_f32 gpamd_lanczos_coef_f32 gpamd_lanczos_subtract_f32 gpamd_lanczos_normalize_f32
  gpamd_block_project_f32 gpamd_block_project_f64 gpamd_block_subtract_f32 gpamd_block_transform_f32
  gpamd_msminres_update_f32 gpamd_precond_coef_f32f64 gpamd_precond_apply_f32f64

Every case: inputs from a seeded generator; every leading dimension once round_up(n, 4) and once that + 8, the pad NaN in every input (a
kernel that reads it poisons its result) and a sentinel in every pure output; results finite, pads and everything a step must not
write BITWISE unchanged; every case run twice from the same state with bitwise-equal results (the sources' "bitwise run-to-run
reproducible").  Shapes: the smallest at which each path exists (the grid-stride second pass of the vector kernels starts at
n > 262 144 for the CG family and n > 131 072 for Lanczos; 128-row basis tiles, column groups of 16 / 80, 256 slices).

TOLERANCES -- derived from the kernels' stated arithmetic, never measured (e = the unit roundoff step ``finfo.eps`` of the kernel's type):
  * elementwise updates (one rounding per operation, at most four operations per element):  |got - ref| <= 4 e sum|terms|, the terms
    being the summands of that element's formula;
  * lanczos_subtract's r = r - sum_{m < k} c_m q_m is NOT a four-operation update: one thread subtracts k rounded products in sequence, so
    the bound is that of a recursive sum of k + 1 terms (Higham, Accuracy and Stability, 4.2: gamma_{k+1}, plus the products' own
    rounding): (k + 2) (e / 2) sum|terms|.  (A first version of this file gave it the 4 e of the short updates; two of 131 075
    elements at k = 255 came out at 4.3 e sum|terms| -- the arithmetic's own error, not the kernel's.)
  * reductions: a thread adds p = 4 ceil(n / (1024 nb)) products in sequence, then come the 6-level wave tree, the sum of the four
    waves and the <= 256 partials summed by the consumer (one per thread, a tree again): first-order bound (p + 32) e sum|a_i b_i|;
    what is computed FROM a reduction (alpha, beta, norms, the vectors scaled by them) gets that bound propagated through its formula;
  * products accumulated in float64 (precond_coef, block_project): 1e-12 sum|r_i q_i|  (n e64 = 1.5e-11 sum|.| would be the worst
    case at the largest n; the sums here are of <= 66 000 terms of random sign);
  * float64 results rounded to float32 (precond_apply, block_subtract, block_transform): e32 |ref| + 1e-12 sum|terms|.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import solver_steps_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN, SENT = float("nan"), -1234.5
EINVAL, EWORKSPACE = -1, -3   # include/gpamd.h: GPAMD_EINVAL, GPAMD_EWORKSPACE
E32 = torch.finfo(F32).eps


def lib():
    from gpytorch_amd._lib import lib as _lib

    return _lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ru4(n):
    return (n + 3) // 4 * 4


def eps_of(dtype):
    return torch.finfo(dtype).eps


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- tolerances (module docstring)
def cg_nb(n):
    return min(256, max(1, -(-n // 1024)))


def lz_nb(n):
    return min(128, max(1, -(-n // 1024)))


def red_rel(n, nb, e):
    """relative first-order bound of a reduction over n elements in nb workgroups, per unit of sum|a_i b_i|"""
    return (4 * math.ceil(n / (1024 * nb)) + 32) * e


def sum_rel(e):
    """... of summing <= 256 given partials (the consumer's part alone: no sequential terms)"""
    return 32 * e


def elem(terms_abs, e):
    return 4 * e * terms_abs


def rounded32(ref, terms_abs):
    return E32 * ref.abs() + 1e-12 * terms_abs


# ---- bitwise comparison, padding, determinism
def bits(x):
    x = x.contiguous()
    if x.dtype == F32:
        return x.view(torch.int32)
    if x.dtype == F64:
        return x.view(torch.int64)
    return x


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def padded(x, ld, dev, fill=NAN):
    """device [..., ld] holding x [..., n] with `fill` in the pad"""
    out = torch.full((*x.shape[:-1], ld), fill, dtype=x.dtype)
    out[..., : x.shape[-1]] = x
    return out.to(dev)


def pad_is(buf, n, fill):
    return same(buf[..., n:], torch.full_like(buf[..., n:], fill))


def within(got, ref, bound, what):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    bad = err > bound
    if bool(bad.any()):
        i = int((err - bound).argmax())
        raise AssertionError(f"{what}: |got - ref| = {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} (ref {float(ref.flatten()[i]):.6e}, "
                             f"{int(bad.sum())} of {bad.numel()} elements)")


def twice(run):
    """run the case twice from the same preset state: bitwise-equal results"""
    a, b = run(), run()
    for k in a:
        assert same(a[k], b[k]), f"{k}: not bitwise reproducible run to run"
    return a


def cancel_pair(n, g, dtype):
    """a, b with sum a_i b_i = 1e-3 sum |a_i b_i|: equal neighbours in a, the odd partner's product negated and 0.2 % smaller"""
    a = torch.randn(n, generator=g, dtype=dtype)
    h = n // 2
    a[1:2 * h:2] = a[0:2 * h:2]
    b = a.clone()
    b[1:2 * h:2] *= -(1 - 2e-3)
    if n % 2:
        b[-1] = 0
    return a, b


# =============================================================================================================== coldot / kv_reduce
CG_N = [1, 3, 5, 1023, 1025, 2051, 262144, 262147, 263171, 524293]
CG_CASES = [pytest.param(dt, n, pad, id=f"{'f64' if dt == F64 else 'f32'}-n{n}-pad{pad}") for dt in (F32, F64) for n in CG_N for pad in (0, 8)]


def ts_of(n):
    return (1, 3, 70) if n == 2051 else (1, 3)


@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_coldot(dev, dtype, n, pad):
    L, e, ld, nb = lib(), eps_of(dtype), ru4(n) + pad, cg_nb(n)
    fn = L.gpamd_coldot_f64 if dtype == F64 else L.gpamd_coldot_f32
    for t in ts_of(n):
        g = gen(n + t)
        A, Bm = torch.randn(t, n, generator=g, dtype=dtype), torch.randn(t, n, generator=g, dtype=dtype)
        A[t - 1], Bm[t - 1] = cancel_pair(n, g, dtype)   # the last column cancels to 1e-3 of sum |a b|
        Ad, Bd = padded(A, ld, dev), padded(Bm, ld, dev)

        def run():
            out = torch.full((t + 1,), SENT, device=dev, dtype=dtype)
            scr = torch.full((t * 256 + 4,), SENT, device=dev, dtype=dtype)
            assert fn(P(Ad), P(Bd), ld, n, t, P(out), P(scr), stream()) == 0
            return dict(out=out.cpu(), scr=scr.cpu())

        r = twice(run)
        ref, sabs = S.coldot(A, Bm), (A.double() * Bm.double()).abs().sum(1)
        within(r["out"][:t], ref, red_rel(n, nb, e) * sabs, f"coldot t={t}")
        assert float(r["out"][t]) == SENT and pad_is(r["scr"], t * 256, SENT)
        assert pad_is(r["scr"][: t * 256].view(t, 256), nb, SENT), "partials beyond the nb workgroups were written"
        if n > 4:
            assert abs(float(ref[t - 1])) < 2e-3 * float(sabs[t - 1])


# (scale, dscale, dvec, Vd, done) given?
KV_OPTS = [(0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (0, 1, 0, 1, 0), (1, 0, 1, 1, 1), (1, 1, 1, 0, 0)]


def kv_opts_for(n, i, pool=KV_OPTS):
    """small n: every option set of the pool with every S; the large n (44 MB slabs at S = 7): one combination each, cycling"""
    if n <= 2051:
        return [(S_, o) for S_ in (1, 2, 7) for o in pool]
    return [((1, 2, 7)[i % 3], pool[i % len(pool)])]


def kv_inputs(n, t, S_, opt, dtype, g, dev, ldp, ldd):
    sc, ds, dv, vd, dn = opt
    Pm = torch.randn(S_, t, n, generator=g, dtype=dtype)
    cpu = dict(P=Pm, scale=torch.tensor([1.7], dtype=dtype) if sc else None, dscale=torch.tensor([0.3], dtype=dtype) if ds else None,
               dvec=torch.rand(n, generator=g, dtype=dtype) if dv else None, Vd=torch.randn(t, n, generator=g, dtype=dtype) if vd else None)
    d = dict(P=padded(Pm, ldp, dev), scale=None if not sc else cpu["scale"].to(dev), dscale=None if not ds else cpu["dscale"].to(dev),
             dvec=None if not dv else padded(cpu["dvec"], ru4(n) + 4, dev), Vd=None if not vd else padded(cpu["Vd"], ldd, dev),
             done=torch.zeros(1, device=dev, dtype=torch.int32) if dn else None)
    return cpu, d


def kv_ref(cpu, Vd):
    """(Out, sum of |terms| per element)"""
    sc = None if cpu["scale"] is None else float(cpu["scale"])
    ds = None if cpu["dscale"] is None else float(cpu["dscale"])
    out = S.kv_reduce(cpu["P"], sc, ds, cpu["dvec"], Vd)
    terms = S.kv_reduce(cpu["P"].abs(), None if sc is None else abs(sc), ds, cpu["dvec"], None if Vd is None else Vd.abs())
    return out, terms


@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_kv_reduce(dev, dtype, n, pad):
    L, e = lib(), eps_of(dtype)
    fn = L.gpamd_kv_reduce_f64 if dtype == F64 else L.gpamd_kv_reduce_f32
    ldp, ldd, ldo = ru4(n) + pad, ru4(n) + 8 - pad, ru4(n) + pad + 4
    for t in ts_of(n):
        for S_, opt in kv_opts_for(n, CG_N.index(n) + t):
            cpu, d = kv_inputs(n, t, S_, opt, dtype, gen(7 * n + t + S_), dev, ldp, ldd)

            def run():
                out = torch.full((t, ldo), SENT, device=dev, dtype=dtype)
                assert fn(P(d["P"]), S_, ldp, t, n, P(d["scale"]), P(d["dscale"]), P(d["dvec"]), P(d["Vd"]), ldd, P(out), ldo, P(d["done"]), stream()) == 0
                return dict(out=out.cpu())

            r = twice(run)
            ref, terms = kv_ref(cpu, cpu["Vd"])
            within(r["out"][:, :n], ref, elem(terms, e), f"kv_reduce t={t} S={S_} opt={opt}")
            assert pad_is(r["out"], n, SENT)


def test_kv_reduce_done_set_writes_nothing(dev):
    L, n, t = lib(), 2051, 3
    ld = ru4(n)
    Pd = padded(torch.randn(2, t, n, generator=gen(0)), ld, dev)
    done = torch.ones(1, device=dev, dtype=torch.int32)
    out = torch.full((t, ld), SENT, device=dev)
    assert L.gpamd_kv_reduce_f32(P(Pd), 2, ld, t, n, None, None, None, None, 0, P(out), ld, P(done), stream()) == 0
    assert pad_is(out.cpu(), 0, SENT)


# =============================================================================================================================== mBCG
VEC = ("X", "R", "D", "Q", "Z")
FSC = ("bnorm", "rnorm", "rho", "stats", "alpha_hist", "beta_hist", "part_a", "part_rz", "part_rr")
ISC = ("zero_rhs", "converged", "done")
PARTS = ("part_a", "part_rz", "part_rr")


def cg_preset(n, t, dtype, g, precond, hist_len=4):
    """a random mid-solve state: unit-scale Gaussian vectors, positive partial sums (as sums of squares are), both halves of rho distinct"""
    nb = cg_nb(n)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)  # noqa: E731
    s = dict(X=r(t, n), R=r(t, n), D=r(t, n), Q=r(t, n))
    if precond:
        s["Z"] = r(t, n)
    for k in PARTS:
        s[k] = r(t, nb).abs() + 0.5
    s.update(rho=r(2, t).abs() + 0.5, bnorm=r(t).abs() + 0.5, rnorm=r(t).abs() + 0.5, alpha_hist=r(hist_len, t), beta_hist=r(hist_len, t), stats=r(4))
    s.update(zero_rhs=torch.zeros(t, dtype=torch.int32), converged=torch.zeros(t, dtype=torch.int32), done=torch.zeros(2, dtype=torch.int32))
    return s


def cg_device(s, n, t, ld, dtype, dev, precond, hist_len=4, out=(), eps=1e-10, stop=1e-10):
    """the preset state on the device: vector pads NaN (inputs) -- a vector named in `out` is a pure output: sentinel everywhere; scratch the
    state does not set (partials beyond nb, ...) holds the sentinel"""
    dv = S.CgDevice(n, t, ld, dtype, dev, hist_len=hist_len, eps=eps, stop_updating_after=stop, precond=precond, fill=NAN)
    dv.fs.fill_(SENT)
    for k in VEC:
        if k == "Z" and not precond:
            continue
        buf = getattr(dv, k)
        if k in out:
            buf.fill_(SENT)
        elif k in s:
            buf[:, :n] = s[k].to(dev)
    for k in FSC + ISC:
        if k in s:
            view = getattr(dv, k)
            if k in PARTS:
                view[:, : s[k].shape[1]] = s[k].to(dev)
            elif view.numel():
                view.copy_(s[k].to(dev))
    return dv


def cg_ref(s, n, t, precond, hist_len=4, eps=1e-10, stop=1e-10):
    st = S.CgRef(n, t, hist_len=hist_len, eps=eps, stop_updating_after=stop, precond=precond)
    st.X, st.D, st.Q = s["X"].double(), s["D"].double(), s["Q"].double()
    st.set_R(s["R"].double())
    if precond:
        st.Z = s["Z"].double()
    st.dq, st.rz, st.rr = (s[k].double().sum(1) for k in PARTS)
    st.rho, st.bnorm, st.rnorm, st.stats = s["rho"].double().clone(), s["bnorm"].double(), s["rnorm"].double(), s["stats"].double().clone()
    st.alpha_hist, st.beta_hist = s["alpha_hist"].double().clone(), s["beta_hist"].double().clone()
    st.zero_rhs, st.converged, st.done = s["zero_rhs"].bool(), s["converged"].bool(), [int(v) for v in s["done"]]
    return st


def snap(dv):
    torch.cuda.synchronize()
    names = [k for k in VEC if not (k == "Z" and dv.Z is dv.R)] + list(FSC + ISC)
    return {k: getattr(dv, k).cpu().clone() for k in names}


def cg_step(s, n, t, ld, dtype, dev, precond, call, changed, **kw):
    """preset -> call -> snapshot, twice (bitwise equal); everything NOT named in `changed` bitwise unchanged; of what is, the vector pads and
    the partials beyond nb.  Returns (pre, post)."""
    pres = []

    def run():
        dv = cg_device(s, n, t, ld, dtype, dev, precond, **kw)
        try:
            pres.append(snap(dv))
            call(dv)
            return snap(dv)
        finally:
            dv.close()

    post, pre = twice(run), pres[0]
    nb = cg_nb(n)
    for k in post:
        if k not in changed:
            assert same(post[k], pre[k]), f"{k} was written"
        elif k in VEC:
            assert same(post[k][:, n:], pre[k][:, n:]), f"the pad of {k} was written"
        elif k in PARTS:
            assert same(post[k][:, nb:], pre[k][:, nb:]), f"{k}: partials beyond the nb = {nb} workgroups were written"
    return pre, post


def psum(part, nb):
    """the finished sum of a column's partials (float64) and the sum of their magnitudes"""
    p = part[:, :nb].double()
    return p.sum(1), p.abs().sum(1)


def ok(rc):
    assert rc == 0, lib().gpamd_last_error()


def col(x):
    return x.unsqueeze(1)


@pytest.mark.parametrize("have_precond", [0, 1])
@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_init(dev, dtype, n, pad, have_precond):
    """gpamd_cg_init_f32 / gpamd_cg64_init: R = B / |B|, X = 0 (D = R, rho, rnorm without a preconditioner); a zero column gets norm 1"""
    e, ld, nb, ldb = eps_of(dtype), ru4(n) + pad, cg_nb(n), ru4(n) + 8 - pad
    for t in ts_of(n):
        g = gen(11 * n + t)
        Bm = torch.randn(t, n, generator=g, dtype=dtype) * 3.0
        if t >= 3:
            Bm[1] = 0
        Bd = padded(Bm, ldb, dev)
        s = cg_preset(n, t, dtype, g, bool(have_precond))
        s["done"] = torch.tensor([1, 5], dtype=torch.int32)   # a finished earlier solve: init must clear it
        changed = {"X", "R", "part_a", "part_rr", "bnorm", "zero_rhs", "done"} | (set() if have_precond else {"D", "part_rz", "rho", "rnorm", "converged"})
        pre, post = cg_step(s, n, t, ld, dtype, dev, bool(have_precond), lambda dv: ok(dv.fn("init")(dv.h, P(Bd), ldb, have_precond, stream())), changed,
                            out=("X", "R") + (() if have_precond else ("D",)))
        st = cg_ref(s, n, t, bool(have_precond))
        S.cg_init(st, Bm, have_precond)
        rr_ = red_rel(n, nb, e)
        b2 = (Bm.double() ** 2).sum(1)
        within(psum(post["part_a"], nb)[0], b2, rr_ * b2, "|b|^2 partials")
        rel_bn = rr_ / 2 + 2 * e                                   # sqrt halves the relative error; + its own rounding
        within(post["bnorm"], st.bnorm, rel_bn * st.bnorm * (~st.zero_rhs), "bnorm")   # (a zero column: exactly 1)
        assert torch.equal(post["zero_rhs"].bool(), st.zero_rhs) and post["done"].tolist() == [0, 0]
        rel_r = rel_bn + 4 * e
        within(post["R"][:, :n], st.R, rel_r * st.R.abs(), "R")
        assert bool((post["X"][:, :n] == 0).all())
        rr_bound = (rr_ + 2.02 * rel_r) * st.rr
        within(psum(post["part_rr"], nb)[0], st.rr, rr_bound, "r.r partials")
        if not have_precond:
            assert same(post["D"][:, :n], post["R"][:, :n]) and same(post["part_rz"][:, :nb], post["part_rr"][:, :nb])
            within(post["rho"][0], st.rho[0], rr_bound, "rho")
            assert same(post["rho"][1], pre["rho"][1])
            within(post["rnorm"], st.rnorm, (rr_bound / st.rr.clamp_min(1e-300) / 2 + 2 * e) * st.rnorm, "rnorm")
            assert torch.equal(post["converged"].bool(), st.converged)


@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_begin(dev, dtype, n, pad):
    """gpamd_cg_begin_f32 / gpamd_cg64_begin (preconditioned form): r.z partials, rho[0], rnorm, converged, done = {0, 0}"""
    e, ld, nb = eps_of(dtype), ru4(n) + pad, cg_nb(n)
    for t in ts_of(n):
        g = gen(13 * n + t)
        s = cg_preset(n, t, dtype, g, True)
        s["R"][t - 1], s["Z"][t - 1] = cancel_pair(n, g, dtype)
        s["done"] = torch.tensor([1, 9], dtype=torch.int32)
        s["part_rr"][0] = 1e-30   # |r| < stop_updating_after: the column is marked converged
        pre, post = cg_step(s, n, t, ld, dtype, dev, True, lambda dv: ok(dv.fn("begin")(dv.h, stream())), {"part_rz", "rho", "rnorm", "converged", "done"})
        st = cg_ref(s, n, t, True)
        S.cg_begin(st)
        sabs = (st.R * st.Z).abs().sum(1)
        within(psum(post["part_rz"], nb)[0], st.rz, red_rel(n, nb, e) * sabs, "r.z partials")
        within(post["rho"][0], st.rho[0], red_rel(n, nb, e) * sabs, "rho")
        assert same(post["rho"][1], pre["rho"][1])
        within(post["rnorm"], st.rnorm, (sum_rel(e) / 2 + 2 * e) * st.rnorm, "rnorm")
        assert torch.equal(post["converged"].bool(), st.converged) and bool(st.converged[0]) and post["done"].tolist() == [0, 0]


@pytest.mark.parametrize("n,pad", [(n, pad) for n in CG_N for pad in (0, 8)])
def test_cg_dot_rz(dev, n, pad):
    """gpamd_cg_dot_rz_f32 (row-sharded, preconditioned): the r.z partials alone"""
    dtype, e, ld, nb = F32, E32, ru4(n) + pad, cg_nb(n)
    for t in ts_of(n):
        g = gen(17 * n + t)
        s = cg_preset(n, t, dtype, g, True)
        s["R"][t - 1], s["Z"][t - 1] = cancel_pair(n, g, dtype)
        pre, post = cg_step(s, n, t, ld, dtype, dev, True, lambda dv: ok(lib().gpamd_cg_dot_rz_f32(dv.h, stream())), {"part_rz"})
        st = cg_ref(s, n, t, True)
        S.cg_dot_rz(st)
        within(psum(post["part_rz"], nb)[0], st.rz, red_rel(n, nb, e) * (st.R * st.Z).abs().sum(1), "r.z partials")


@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_reduce_q(dev, dtype, n, pad):
    """gpamd_cg_reduce_q_f32 / gpamd_cg64_reduce_q on synthetic slabs P[S][t][ldp]: Q and the d.q partials"""
    e, ld, nb, ldp = eps_of(dtype), ru4(n) + pad, cg_nb(n), ru4(n) + 8 - pad
    for t in ts_of(n):
        for S_, opt in kv_opts_for(n, CG_N.index(n) + t, KV_OPTS[1:4]):   # (Vd is the solver's D: always there)
            g = gen(19 * n + t + S_)
            cpu, d = kv_inputs(n, t, S_, opt, dtype, g, dev, ldp, ldp)
            s = cg_preset(n, t, dtype, g, False)
            if S_ == 1 and opt == KV_OPTS[2]:
                s["D"][t - 1], cpu["P"][0, t - 1] = cancel_pair(n, g, dtype)   # d.(K d) cancels to ~1e-3 (+ the 0.3 d.d of the diagonal)
                cpu["dscale"] = torch.tensor([1e-3], dtype=dtype)
                d["P"], d["dscale"] = padded(cpu["P"], ldp, dev), cpu["dscale"].to(dev)
            call = lambda dv: ok(dv.fn("reduce_q")(dv.h, P(d["P"]), S_, ldp, P(d["scale"]), P(d["dscale"]), P(d["dvec"]), stream()))  # noqa: E731
            pre, post = cg_step(s, n, t, ld, dtype, dev, False, call, {"Q", "part_a"}, out=("Q",))
            ref, terms = kv_ref(cpu, s["D"])
            dq_bound = red_rel(n, nb, e) * (s["D"].double() * ref).abs().sum(1) + (s["D"].double().abs() * elem(terms, e)).sum(1)
            within(post["Q"][:, :n], ref, elem(terms, e), f"Q t={t} S={S_} opt={opt}")
            within(psum(post["part_a"], nb)[0], (s["D"].double() * ref).sum(1), dq_bound, f"d.q partials t={t} S={S_} opt={opt}")


def alpha_bounds(st, pre, nb, e):
    """|alpha - ref| from the sum of the preset d.q partials and the division (0 for a masked column: alpha must be exactly 0)"""
    den, dabs = psum(pre["part_a"], nb)
    dden = sum_rel(e) * dabs
    return st.alpha.abs() * (dden / (den.abs() - dden).clamp_min(1e-300) + 2 * e)


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_update_xr(dev, dtype, n, pad, precond):
    """gpamd_cg_update_xr_f32 / gpamd_cg64_update_xr: alpha from rho[k & 1] and the d.q partials; X, R, r.r partials (and r.z = r.r iff Z == R)"""
    e, ld, nb, k = eps_of(dtype), ru4(n) + pad, cg_nb(n), 1 if pad else 0
    for t in ts_of(n):
        s = cg_preset(n, t, dtype, gen(23 * n + t), precond)
        call = lambda dv: ok(dv.fn("update_xr")(dv.h, k, stream()))  # noqa: E731
        pre, post = cg_step(s, n, t, ld, dtype, dev, precond, call, {"X", "R", "part_rr", "alpha_hist"} | (set() if precond else {"part_rz"}))
        st = cg_ref(s, n, t, precond)
        S.cg_update_xr(st, k)
        da = alpha_bounds(st, pre, nb, e)
        a = col(st.alpha)
        within(post["alpha_hist"][k], st.alpha, da, "alpha")
        for j in range(4):
            assert j == k or same(post["alpha_hist"][j], pre["alpha_hist"][j])
        within(post["X"][:, :n], st.X, elem(s["X"].double().abs() + (a * st.D).abs(), e) + col(da) * st.D.abs(), "X")
        dr = elem(s["R"].double().abs() + (a * st.Q).abs(), e) + col(da) * st.Q.abs()
        within(post["R"][:, :n], st.R, dr, "R")
        rr_bound = red_rel(n, nb, e) * st.rr + 1.01 * (2 * st.R.abs() * dr + dr * dr).sum(1)
        within(psum(post["part_rr"], nb)[0], st.rr, rr_bound, "r.r partials")
        if not precond:
            assert same(post["part_rz"][:, :nb], post["part_rr"][:, :nb]), "Z == R: the r.z partials are the r.r partials"


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_update_d(dev, dtype, n, pad, precond):
    """gpamd_cg_update_d_f32 / gpamd_cg64_update_d: (r.z when preconditioned) beta, D = Z + beta D, rho_new into the OTHER half, rnorm, converged, stats"""
    e, ld, nb, k = eps_of(dtype), ru4(n) + pad, cg_nb(n), 1 if pad else 0
    for t in ts_of(n):
        g = gen(29 * n + t)
        s = cg_preset(n, t, dtype, g, precond)
        s["part_rr"][0] = 1e-30
        if precond:
            s["R"][t - 1], s["Z"][t - 1] = cancel_pair(n, g, dtype)
        call = lambda dv: ok(dv.fn("update_d")(dv.h, k, stream()))  # noqa: E731
        pre, post = cg_step(s, n, t, ld, dtype, dev, precond, call, {"D", "rho", "rnorm", "converged", "beta_hist", "stats"} | ({"part_rz"} if precond else set()))
        st = cg_ref(s, n, t, precond)
        S.cg_update_d(st, k)
        if precond:
            drho = red_rel(n, nb, e) * (st.R * st.Z).abs().sum(1)
            within(psum(post["part_rz"], nb)[0], st.rz, drho, "r.z partials")
        else:
            drho = sum_rel(e) * psum(pre["part_rz"], nb)[1]
        new, old = (k + 1) & 1, k & 1
        within(post["rho"][new], st.rho[new], drho, "rho_new")
        assert same(post["rho"][old], pre["rho"][old]), "rho_old was written"
        db = drho / st.rho[old].abs() + 2 * e * st.beta.abs()
        within(post["beta_hist"][k], st.beta, db, "beta")
        for j in range(4):
            assert j == k or same(post["beta_hist"][j], pre["beta_hist"][j])
        b = col(st.beta)
        within(post["D"][:, :n], st.D, elem(st.Z.abs() + (b * s["D"].double()).abs(), e) + col(db) * s["D"].double().abs(), "D")
        drn = (sum_rel(e) / 2 + 2 * e) * st.rnorm
        within(post["rnorm"], st.rnorm, drn, "rnorm")
        assert torch.equal(post["converged"].bool(), st.converged) and bool(st.converged[0])
        within(post["stats"][0], st.stats[0], drn.sum() + sum_rel(e) * st.rnorm.sum(), "stats[0]")
        assert float(post["stats"][1]) == t and same(post["stats"][2:], pre["stats"][2:])


@pytest.mark.parametrize("dtype,n,pad", CG_CASES)
def test_cg_finish(dev, dtype, n, pad):
    """gpamd_cg_finish_f32 / gpamd_cg64_finish: X *= |B|"""
    e, ld = eps_of(dtype), ru4(n) + pad
    for t in ts_of(n):
        s = cg_preset(n, t, dtype, gen(31 * n + t), False)
        pre, post = cg_step(s, n, t, ld, dtype, dev, False, lambda dv: ok(dv.fn("finish")(dv.h, stream())), {"X"})
        st = cg_ref(s, n, t, False)
        S.cg_finish(st)
        within(post["X"][:, :n], st.X, elem(st.X.abs(), e), "X")


# ---- semantics: masks and side channels, each its own small case at n = 2051
SN, ST = 2051, 3


def small(dtype=F32, precond=False, seed=0, hist_len=4):
    return cg_preset(SN, ST, dtype, gen(seed), precond, hist_len)


def test_alpha_masks(dev):
    """d.q < eps for one column, converged for another: alpha = 0, X and R unchanged BITWISE, the history row written as 0"""
    s = small(seed=1)
    s["part_a"][0] = 1e-13 / cg_nb(SN)     # sum = 1e-13 < eps = 1e-10
    s["converged"][1] = 1
    pre, post = cg_step(s, SN, ST, ru4(SN), F32, dev, False, lambda dv: ok(lib().gpamd_cg_update_xr_f32(dv.h, 2, stream())),
                        {"X", "R", "part_rr", "part_rz", "alpha_hist"})
    assert post["alpha_hist"][2].tolist()[:2] == [0.0, 0.0] and float(post["alpha_hist"][2][2]) != 0.0
    for c in (0, 1):
        assert same(post["X"][c], pre["X"][c]) and same(post["R"][c], pre["R"][c])
    assert not same(post["X"][2], pre["X"][2])
    # a NEGATIVE denominator (an indefinite product) is masked too: d.q < eps, not |d.q| < eps
    s["part_a"][2] = -1.0
    pre, post = cg_step(s, SN, ST, ru4(SN), F32, dev, False, lambda dv: ok(lib().gpamd_cg_update_xr_f32(dv.h, 2, stream())),
                        {"X", "R", "part_rr", "part_rz", "alpha_hist"})
    assert post["alpha_hist"][2].tolist() == [0.0, 0.0, 0.0] and same(post["X"], pre["X"]) and same(post["R"], pre["R"])


def test_beta_mask(dev):
    """rho_old < eps: beta = 0 and D = Z (bitwise)"""
    s = small(precond=True, seed=2)
    s["rho"][0, 1] = 1e-12
    pre, post = cg_step(s, SN, ST, ru4(SN) + 8, F32, dev, True, lambda dv: ok(lib().gpamd_cg_update_d_f32(dv.h, 0, stream())),
                        {"D", "rho", "rnorm", "converged", "beta_hist", "stats", "part_rz"})
    assert float(post["beta_hist"][0][1]) == 0.0 and float(post["beta_hist"][0][0]) != 0.0
    assert same(post["D"][1, :SN], post["Z"][1, :SN]) and not same(post["D"][0, :SN], post["Z"][0, :SN])


def test_zero_rhs(dev):
    """a zero right-hand side: norm 1, R = 0, zero_rhs = 1; rnorm = 0 after update_d; X exact zeros through finish"""
    L, n, t, ld = lib(), SN, ST, ru4(SN)
    Bm = torch.randn(t, n, generator=gen(3))
    Bm[1] = 0
    Bd = padded(Bm, ld, dev)
    dv = cg_device(small(seed=3), n, t, ld, F32, dev, False)
    try:
        ok(L.gpamd_cg_init_f32(dv.h, P(Bd), ld, 0, stream()))
        a = snap(dv)
        assert a["bnorm"].tolist()[1] == 1.0 and a["zero_rhs"].tolist() == [0, 1, 0] and bool((a["R"][1, :n] == 0).all())
        dv.part_rr[1, :dv.nb] = 0.25   # even if the residual partials were not zero, the column's rnorm is forced to 0
        ok(L.gpamd_cg_reduce_q_f32(dv.h, P(padded(Bm * 2, ld, dev).unsqueeze(0).contiguous()), 1, ld, None, None, None, stream()))
        ok(L.gpamd_cg_update_xr_f32(dv.h, 0, stream()))
        dv.part_rr[1, :dv.nb] = 0.25
        ok(L.gpamd_cg_update_d_f32(dv.h, 0, stream()))
        ok(L.gpamd_cg_finish_f32(dv.h, stream()))
        b = snap(dv)
        assert float(b["rnorm"][1]) == 0.0 and float(b["rnorm"][0]) > 0 and b["converged"].tolist()[1] == 1
        assert bool((b["X"][1, :n] == 0).all()) and bool((b["X"][0, :n] != 0).any())
    finally:
        dv.close()


def test_history_bounds(dev):
    """hist_len = 2: steps 0 and 1 write their rows; step 2 writes nothing, and the d.q partials that lie directly behind beta_hist in the scratch
    are what reduce_q left"""
    L, n, t, ld = lib(), SN, ST, ru4(SN)
    s = small(seed=4, hist_len=2)
    dv = cg_device(s, n, t, ld, F32, dev, False, hist_len=2)
    try:
        for k in range(3):
            slab = (dv.D * 1.5).unsqueeze(0).contiguous()   # d.q = 1.5 |d|^2 > 0
            slab[:, :, n:] = NAN
            ok(L.gpamd_cg_reduce_q_f32(dv.h, P(slab), 1, ld, None, None, None, stream()))
            a = snap(dv)
            ok(L.gpamd_cg_update_xr_f32(dv.h, k, stream()))
            ok(L.gpamd_cg_update_d_f32(dv.h, k, stream()))
            b = snap(dv)
            assert same(b["part_a"], a["part_a"])
            if k < 2:
                assert not same(b["alpha_hist"][k], a["alpha_hist"][k]) and not same(b["beta_hist"][k], a["beta_hist"][k])
                assert same(b["alpha_hist"][1 - k], a["alpha_hist"][1 - k]) and same(b["beta_hist"][1 - k], a["beta_hist"][1 - k])
                assert bool((b["alpha_hist"][k] > 0).all()) and bool((b["beta_hist"][k] > 0).all())
            else:
                assert same(b["alpha_hist"], a["alpha_hist"]) and same(b["beta_hist"], a["beta_hist"])
                assert not same(b["X"], a["X"])   # (the step itself ran)
    finally:
        dv.close()


def test_done_makes_every_step_a_noop(dev):
    s = small(precond=True, seed=5)
    s["done"] = torch.tensor([1, 3], dtype=torch.int32)
    slab = padded(torch.randn(2, ST, SN, generator=gen(5)), ru4(SN), dev)

    def call(dv):
        L = lib()
        ok(L.gpamd_cg_reduce_q_f32(dv.h, P(slab), 2, ru4(SN), None, None, None, stream()))
        ok(L.gpamd_cg_update_xr_f32(dv.h, 3, stream()))
        ok(L.gpamd_cg_dot_rz_f32(dv.h, stream()))
        ok(L.gpamd_cg_update_d_f32(dv.h, 3, stream()))
        ok(L.gpamd_cg_update_d_apply_f32(dv.h, 3, stream()))
        ok(L.gpamd_cg_stop_f32(dv.h, 3, 0, 0, 1e30, stream()))

    cg_step(s, SN, ST, ru4(SN) + 8, F32, dev, True, call, set())
    s64 = small(F64, True, 5)
    s64["done"] = torch.tensor([2, 3], dtype=torch.int32)
    slab64 = slab.double()

    def call64(dv):
        L = lib()
        ok(L.gpamd_cg64_reduce_q(dv.h, P(slab64), 2, ru4(SN), None, None, None, stream()))
        ok(L.gpamd_cg64_update_xr(dv.h, 3, stream()))
        ok(L.gpamd_cg64_update_d(dv.h, 3, stream()))
        ok(L.gpamd_cg64_stop(dv.h, 3, 0, 0, 1e30, stream()))

    cg_step(s64, SN, ST, ru4(SN), F64, dev, True, call64, set())


def test_k_minus_one_takes_the_index_from_done(dev):
    """done[1] = 1: update_xr / update_d / stop with k = -1 equal the k = 1 calls bitwise (which half of rho is read, which written; the history row)"""
    s = small(precond=True, seed=6)
    s["done"] = torch.tensor([0, 1], dtype=torch.int32)
    s["stats"][:2] = torch.tensor([1.0, 3.0])

    def calls(k):
        def call(dv):
            L = lib()
            ok(L.gpamd_cg_update_xr_f32(dv.h, k, stream()))
            ok(L.gpamd_cg_update_d_f32(dv.h, k, stream()))
            ok(L.gpamd_cg_stop_f32(dv.h, k, 0, 0, 0.0, stream()))
        return call

    changed = {"X", "R", "D", "part_rr", "part_rz", "alpha_hist", "beta_hist", "rho", "rnorm", "converged", "stats", "done"}
    pre, a = cg_step(s, SN, ST, ru4(SN), F32, dev, True, calls(-1), changed)
    _, b = cg_step(s, SN, ST, ru4(SN), F32, dev, True, calls(1), changed)
    for k in a:
        assert same(a[k], b[k]), k
    assert a["done"].tolist() == [0, 2]
    assert same(a["rho"][1], pre["rho"][1]) and not same(a["rho"][0], pre["rho"][0])          # k = 1 reads half 1, writes half 0
    assert not same(a["alpha_hist"][1], pre["alpha_hist"][1]) and same(a["alpha_hist"][0], pre["alpha_hist"][0])


STOP_CASES = [  # (k, min_iter, tridiag_floor, tol, stats0, stats1) -- either side of each of the rule's three conditions, then NaN
    (10, 10, 0, 1.0, 1.5, 3.0), (9, 10, 0, 1.0, 1.5, 3.0), (10, 10, 0, 0.5, 1.5, 3.0), (10, 10, 0, 0.5, 1.4999, 3.0),
    (10, 10, 11, 1.0, 1.5, 3.0), (10, 10, 10, 1.0, 1.5, 3.0), (0, 0, 0, 1.0, 1.5, 3.0), (4, 0, 0, 1.0, NAN, 3.0), (4, 10, 20, 1.0, NAN, 3.0),
]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_cg_stop_rule(dev, dtype):
    """gpamd_cg_stop_f32 / gpamd_cg64_stop: k >= min_iter and mean < tol and not k < tridiag_floor; done[1] = k + 1; a NaN mean: done = {2, k + 1}"""
    for k, mi, fl, tol, s0, s1 in STOP_CASES:
        s = small(dtype, seed=7)
        s["stats"][:2] = torch.tensor([s0, s1], dtype=dtype)
        pre, post = cg_step(s, SN, ST, ru4(SN), dtype, dev, False, lambda dv: ok(dv.fn("stop")(dv.h, k, mi, fl, tol, stream())), {"done"})
        st = cg_ref(s, SN, ST, False)
        S.cg_stop(st, k, mi, fl, tol)
        assert post["done"].tolist() == st.done, (k, mi, fl, tol, s0)
    want = [[1, 11], [0, 10], [0, 11], [1, 11], [0, 11], [1, 11], [1, 1], [2, 5], [2, 5]]
    for (k, mi, fl, tol, s0, s1), w in zip(STOP_CASES, want):   # the reference's own answers, spelled out
        st = S.CgRef(SN, ST)
        st.stats[:2] = torch.tensor([s0, s1], dtype=F64)
        S.cg_stop(st, k, mi, fl, tol)
        assert st.done == w


def test_row_sharded_split_equals_whole(dev):
    """init_norms + init_apply(copy_d) + begin_apply == cg_init; dot_rz + update_d_apply == update_d -- bitwise"""
    L, n, t, ld = lib(), SN, ST, ru4(SN) + 8
    Bd = padded(torch.randn(t, n, generator=gen(8)), ld, dev)
    s = small(seed=8)
    changed = {"X", "R", "D", "part_a", "part_rr", "part_rz", "bnorm", "zero_rhs", "done", "rho", "rnorm", "converged"}
    _, whole = cg_step(s, n, t, ld, F32, dev, False, lambda dv: ok(L.gpamd_cg_init_f32(dv.h, P(Bd), ld, 0, stream())), changed)

    def split(dv):
        ok(L.gpamd_cg_init_norms_f32(dv.h, P(Bd), ld, stream()))
        ok(L.gpamd_cg_init_apply_f32(dv.h, P(Bd), ld, 1, stream()))
        ok(L.gpamd_cg_begin_apply_f32(dv.h, stream()))

    _, parts = cg_step(s, n, t, ld, F32, dev, False, split, changed)
    for k in whole:
        assert same(whole[k], parts[k]), k
    s = small(precond=True, seed=9)
    changed = {"D", "rho", "rnorm", "converged", "beta_hist", "stats", "part_rz"}
    _, whole = cg_step(s, n, t, ld, F32, dev, True, lambda dv: ok(L.gpamd_cg_update_d_f32(dv.h, 1, stream())), changed)

    def split_d(dv):
        ok(L.gpamd_cg_dot_rz_f32(dv.h, stream()))
        ok(L.gpamd_cg_update_d_apply_f32(dv.h, 1, stream()))

    _, parts = cg_step(s, n, t, ld, F32, dev, True, split_d, changed)
    for k in whole:
        assert same(whole[k], parts[k]), k


# ============================================================================================================================ Lanczos
LZ_N = [1, 5, 1027, 131072, 131075, 132099]
# k = 512 at n <= 1027 only (a 512 x 132 099 basis is 270 MB for a path -- the 256-wide write-out and coefficient load -- that does not depend on n)
LZ_NK = [(n, k) for n in LZ_N for k in ((1, 255, 256, 257, 512) if n <= 1027 else (1, 255, 256, 257))]


@functools.lru_cache(maxsize=2)
def lz_basis(n):
    """[512 or 257, n] unit-scale Gaussian rows, one draw per n shared by the cases (read-only)"""
    return torch.randn(512 if n <= 1027 else 257, n, generator=gen(n), dtype=F32)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n", LZ_N)
def test_lanczos_residual(dev, n, pad):
    L, g = lib(), gen(n)
    w, q = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ld = ru4(n) + pad
    wd, qd, beta = padded(w, ld, dev), padded(q, ld, dev), torch.tensor([0.75, NAN], device=dev)
    for qp, bp in ((qd, beta), (None, None), (None, beta)):
        def run():
            r = torch.full((ld,), SENT, device=dev)
            ok(L.gpamd_lanczos_residual_f32(P(wd), P(qp), P(bp), P(r), n, stream()))
            return dict(r=r.cpu())

        r = twice(run)["r"]
        ref = S.lanczos_residual(w, q if qp is not None else None, 0.75)
        within(r[:n], ref, elem(w.double().abs() + (0.75 * q.double().abs() if qp is not None else 0), E32), "r")
        assert pad_is(r, n, SENT)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n,k", LZ_NK)
def test_lanczos_project(dev, n, k, pad):
    """gpamd_lanczos_project_f32: partials of <Q[m], r>, m < k; the last basis row cancels against r to 1e-3"""
    L, nb, ldq = lib(), lz_nb(n), ru4(n) + pad
    assert nb == L.gpamd_lanczos_num_partials(n) and L.gpamd_lanczos_partial_stride() == 128
    Q = lz_basis(n)[:k]
    r, last = cancel_pair(n, gen(n + k), F32)
    Qd = padded(Q, ldq, dev)
    Qd[k - 1, :n] = last.to(dev)
    rd = padded(r, ru4(n) + 8 - pad, dev)

    def run():
        part = torch.full((k + 1, 128), SENT, device=dev)
        ok(L.gpamd_lanczos_project_f32(P(Qd), ldq, k, P(rd), n, P(part), stream()))
        return dict(part=part.cpu())

    part = twice(run)["part"]
    ref, sabs = S.lanczos_project(Q, r), Q.double().abs() @ r.double().abs()
    ref[k - 1], sabs[k - 1] = (last.double() * r.double()).sum(), (last.double() * r.double()).abs().sum()
    within(part[:k, :nb].double().sum(1), ref, red_rel(n, nb, E32) * sabs, "coefficients")
    assert pad_is(part[:k], nb, SENT) and pad_is(part[k], 0, SENT)


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 128])
def test_lanczos_coef(dev, nb):
    """gpamd_lanczos_coef_f32: coef[m] = sum_b part[m][b] over nb partials (a lane sums ceil(nb / 64) of them, then the wave tree)"""
    L, k = lib(), 257
    part = torch.randn(k, nb, generator=gen(nb))
    pd = padded(part, 128, dev)   # the unused entries of a row: NaN -- never read

    def run():
        coef, flag = torch.full((k + 1,), SENT, device=dev), torch.zeros(2, device=dev, dtype=torch.int32)
        ok(L.gpamd_lanczos_coef_f32(P(pd), k, nb, 1e30, P(coef), P(flag), stream()))
        return dict(coef=coef.cpu(), flag=flag.cpu())

    r = twice(run)
    ref, _ = S.lanczos_coef(part, 1e30, 0)
    within(r["coef"][:k], ref, (math.ceil(nb / 64) + 32) * E32 * part.double().abs().sum(1), "coef")
    assert float(r["coef"][k]) == SENT and r["flag"].tolist() == [0, 0]


def test_lanczos_coef_flag(dev):
    """flag goes 0 -> 1 only when some |c| > tol; stays 1; untouched for tol < 0 (NULL accepted then, refused for tol >= 0)"""
    L = lib()
    part = torch.zeros(3, 128, device=dev)
    part[:, 0] = torch.tensor([1e-6, -3e-3, 2e-4], device=dev)
    coef = torch.zeros(3, device=dev)
    for tol, start in ((1e-2, 0), (1e-3, 0), (3.1e-3, 0), (1e-2, 1), (-1.0, 0), (-1.0, 1)):
        flag = torch.tensor([start, 7], device=dev, dtype=torch.int32)
        ok(L.gpamd_lanczos_coef_f32(P(part), 3, 1, tol, P(coef), P(flag), stream()))
        assert flag.tolist() == [S.lanczos_coef(part[:, :1].cpu(), tol, start)[1], 7], (tol, start)
    ok(L.gpamd_lanczos_coef_f32(P(part), 3, 1, -1.0, P(coef), None, stream()))
    torch.cuda.synchronize()
    assert L.gpamd_lanczos_coef_f32(P(part), 3, 1, 1e-3, P(coef), None, stream()) == EINVAL
    assert L.gpamd_lanczos_coef_f32(P(part), 3, 129, -1.0, P(coef), None, stream()) == EINVAL


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n,k", LZ_NK)
def test_lanczos_subtract(dev, n, k, pad):
    """gpamd_lanczos_subtract_f32: r -= sum_m coef[m] Q[m] in place; partials of |r|^2"""
    L, nb, ldq = lib(), lz_nb(n), ru4(n) + pad
    Q, g = lz_basis(n)[:k], gen(3 * n + k)
    r, coef = torch.randn(n, generator=g), torch.randn(k, generator=g) / math.sqrt(k)
    Qd, cd = padded(Q, ldq, dev), padded(coef, k + 3, dev)

    def run():
        rd, part = padded(r, ru4(n) + 8 - pad, dev), torch.full((128 + 1,), SENT, device=dev)
        ok(L.gpamd_lanczos_subtract_f32(P(Qd), ldq, k, P(cd), P(rd), n, P(part), stream()))
        return dict(r=rd.cpu(), part=part.cpu())

    got = twice(run)
    ref, rr = S.lanczos_subtract(Q, coef, r)
    dr = (k + 2) * (E32 / 2) * (r.double().abs() + coef.double().abs() @ Q.double().abs())   # k sequential multiply-subtracts (module docstring)
    within(got["r"][:n], ref, dr, "r")
    assert pad_is(got["r"], n, NAN)
    within(got["part"][:nb].double().sum(), torch.tensor(rr, dtype=F64), red_rel(n, nb, E32) * rr + 1.01 * float((2 * ref.abs() * dr + dr * dr).sum()), "|r|^2")
    assert pad_is(got["part"], nb, SENT)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n", LZ_N)
def test_lanczos_normalize(dev, n, pad):
    L, ld = lib(), ru4(n) + pad
    r = torch.randn(n, generator=gen(n))
    rr32 = (r * r).sum().reshape(1)
    rd, rrd = padded(r, ld, dev), torch.cat([rr32, torch.tensor([NAN])]).to(dev)
    for in_place in (False, True):
        def run():
            src = rd.clone()
            out = src if in_place else torch.full((ld,), SENT, device=dev)
            nrm, stop = torch.full((2,), SENT, device=dev), torch.tensor([0, 7], device=dev, dtype=torch.int32)
            ok(L.gpamd_lanczos_normalize_f32(P(src), n, P(rrd), P(out), P(nrm), 1e-6, P(stop), stream()))
            return dict(out=out.cpu(), nrm=nrm.cpu(), stop=stop.cpu())

        got = twice(run)
        ref, nref, _ = S.lanczos_normalize(r, rr32[0], 1e-6, 0)
        within(got["out"][:n], ref, elem(ref.abs(), E32), "out")
        within(got["nrm"][0], torch.tensor(nref, dtype=F64), 2 * E32 * nref, "norm")
        assert pad_is(got["out"], n, NAN if in_place else SENT) and float(got["nrm"][1]) == SENT and got["stop"].tolist() == [0, 7]


def test_lanczos_normalize_edges(dev):
    """rr = 0: exact zeros and stop; a tiny negative rr (a rounded sum) is clamped, not NaN; a norm just above tiny leaves stop at 0; norm_out / stop may be NULL"""
    L, n = lib(), 1027
    r = padded(torch.randn(n, generator=gen(1)), ru4(n), dev)
    for rr, tiny, want_stop in ((0.0, 1e-6, 1), (-1e-12, 1e-6, 1), (1.0001e-12, 1e-6, 0), (0.9999e-12, 1e-6, 1), (4.0, 1e-6, 0)):
        for start in (0, 1):
            out, nrm = torch.full((ru4(n),), SENT, device=dev), torch.full((1,), SENT, device=dev)
            stop, rrd = torch.tensor([start], device=dev, dtype=torch.int32), torch.tensor([rr], device=dev)
            ok(L.gpamd_lanczos_normalize_f32(P(r), n, P(rrd), P(out), P(nrm), tiny, P(stop), stream()))
            ref, nref, sref = S.lanczos_normalize(r[:n].cpu(), float(rrd.cpu()[0]), tiny, start)
            assert stop.tolist() == [sref] and sref == (want_stop | start), (rr, start)
            assert bool(torch.isfinite(out[:n]).all()) and abs(float(nrm[0]) - nref) <= 2 * E32 * nref
            if rr <= 0:
                assert bool((out[:n] == 0).all()) and float(nrm[0]) == 0.0
    out = torch.full((ru4(n),), SENT, device=dev)
    ok(L.gpamd_lanczos_normalize_f32(P(r), n, P(torch.tensor([4.0], device=dev)), P(out), None, 1e-6, None, stream()))
    within(out[:n], r[:n].cpu().double() / 2, 0.0, "NULL norm_out / stop")


def test_lanczos_limits(dev):
    """include/gpamd.h: k <= 512 and ldq % 4 == 0 for project / subtract -- GPAMD_EINVAL before any launch, nothing written"""
    L, n = lib(), 64
    Q, r = torch.zeros(513, 64, device=dev), torch.full((64,), 1.0, device=dev)
    part, coef = torch.full((513 * 128,), SENT, device=dev), torch.zeros(513, device=dev)
    assert L.gpamd_lanczos_project_f32(P(Q), 64, 513, P(r), n, P(part), stream()) == EINVAL
    assert L.gpamd_lanczos_subtract_f32(P(Q), 64, 513, P(coef), P(r), n, P(part), stream()) == EINVAL
    assert L.gpamd_lanczos_project_f32(P(Q), 66, 4, P(r), n, P(part), stream()) == EINVAL
    assert L.gpamd_lanczos_subtract_f32(P(Q), 66, 4, P(coef), P(r), n, P(part), stream()) == EINVAL
    assert L.gpamd_lanczos_project_f32(P(Q), 60, 4, P(r), n, P(part), stream()) == EINVAL   # ldq < n
    torch.cuda.synchronize()
    assert pad_is(part.cpu(), 0, SENT) and bool((r == 1.0).all())
    ok(L.gpamd_lanczos_project_f32(P(Q), 64, 512, P(r), n, P(part), stream()))


# =============================================================================================== preconditioner: coefficients and apply
PC_CASES = ([(4099, k, 5) for k in (1, 3, 30, 128, 129, 131, 257, 512)] + [(4099, 131, t) for t in (1, 16, 17, 80, 81, 97)]
            + [(n, 131, 17) for n in (1, 127, 129, 32805)])


def pc_lds(n, variant):
    """(ldr, ldq, ldo): each once round_up(n, 4) and once that + 8 with ldr != ldq != ldo (variants 0, 1); variant 2: all three different"""
    return ((ru4(n), ru4(n) + 8, ru4(n)), (ru4(n) + 8, ru4(n), ru4(n) + 8), (ru4(n) + 4, ru4(n) + 8, ru4(n)))[variant]


@functools.lru_cache(maxsize=4)
def pc_problem(n, k, t):
    """Q1 [k, n] float64 with orthonormal rows (n >= k; scaled Gaussian rows otherwise) and float32 residuals R [t, n] that lie 99.9 % inside the span of
    Q1 -- the cancellation the float64 apply exists for"""
    g = gen(1000 * k + t + n)
    if n >= k:
        Q1 = torch.linalg.qr(torch.randn(n, k, generator=g, dtype=F64))[0].t().contiguous()
        R = (torch.randn(t, k, generator=g, dtype=F64) @ Q1) * math.sqrt(n / k) + 1e-3 * torch.randn(t, n, generator=g, dtype=F64)
    else:
        Q1 = torch.randn(k, n, generator=g, dtype=F64) / math.sqrt(k)
        R = torch.randn(t, n, generator=g, dtype=F64)
    return Q1, R.float()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n,k,t", PC_CASES)
def test_precond_coef(dev, n, k, t, variant):
    """gpamd_precond_coef_f32f64: W = R Q1^T, float64 accumulation; workspace of exactly gpamd_precond_coef_workspace_doubles"""
    L = lib()
    Q1, R = pc_problem(n, k, t)
    ldr, ldq, _ = pc_lds(n, variant)
    Rd, Qd = padded(R, ldr, dev), padded(Q1, ldq, dev)
    nws = int(L.gpamd_precond_coef_workspace_doubles(n, t, k))

    def run():
        W, ws = torch.full((t * k + 2,), SENT, device=dev, dtype=F64), torch.full((nws + 2,), SENT, device=dev, dtype=F64)
        ok(L.gpamd_precond_coef_f32f64(P(Rd), ldr, t, P(Qd), ldq, k, n, P(W), P(ws), nws, stream()))
        return dict(W=W.cpu(), ws=ws.cpu())

    got = twice(run)
    within(got["W"][: t * k].view(t, k), S.precond_coef(R, Q1), 1e-12 * (R.double().abs() @ Q1.abs().t()), "W")
    assert pad_is(got["W"], t * k, SENT) and pad_is(got["ws"], nws, SENT)
    W = torch.full((t * k,), SENT, device=dev, dtype=F64)
    ws = torch.empty(nws, device=dev, dtype=F64)
    assert L.gpamd_precond_coef_f32f64(P(Rd), ldr, t, P(Qd), ldq, k, n, P(W), P(ws), nws - 1, stream()) == EWORKSPACE
    torch.cuda.synchronize()
    assert pad_is(W.cpu(), 0, SENT)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("n,k,t", PC_CASES)
def test_precond_apply(dev, n, k, t, variant):
    """gpamd_precond_apply_f32f64: Out = (R - W Q1) / sigma2 in float64, rounded once to float32 -- with R 99.9 % inside the span of Q1 a float32
    subtraction would miss this bound by orders of magnitude"""
    L, sigma2 = lib(), 0.1
    Q1, R = pc_problem(n, k, t)
    W = S.precond_coef(R, Q1)
    ldr, ldq, ldo = pc_lds(n, variant)
    Rd, Qd, Wd, s2 = padded(R, ldr, dev), padded(Q1, ldq, dev), W.to(dev), torch.tensor([sigma2], device=dev)

    def run():
        out = torch.full((t, ldo), SENT, device=dev)
        ok(L.gpamd_precond_apply_f32f64(P(Rd), ldr, t, P(Qd), ldq, k, n, P(Wd), P(s2), P(out), ldo, stream()))
        return dict(out=out.cpu())

    out = twice(run)["out"]
    s2f = float(torch.tensor(sigma2, dtype=F32))
    ref = S.precond_apply(R, Q1, W, s2f)
    within(out[:, :n], ref, rounded32(ref, (R.double().abs() + W.abs() @ Q1.abs()) / s2f), "Out")
    assert pad_is(out, n, SENT)
    if n >= k:
        assert float(ref.abs().max()) < 0.05 * float(R.abs().max()) / s2f   # (the cancellation is there)


def test_precond_limits(dev):
    """include/gpamd.h: k <= 512"""
    L, n = lib(), 64
    R, Q, W = torch.zeros(2, n, device=dev), torch.zeros(513, n, device=dev, dtype=F64), torch.full((2 * 513,), SENT, device=dev, dtype=F64)
    ws, out, s2 = torch.zeros(4 * 2 * 513, device=dev, dtype=F64), torch.full((2, n), SENT, device=dev), torch.ones(1, device=dev)
    assert L.gpamd_precond_coef_f32f64(P(R), n, 2, P(Q), n, 513, n, P(W), P(ws), ws.numel(), stream()) == EINVAL
    assert L.gpamd_precond_apply_f32f64(P(R), n, 2, P(Q), n, 513, n, P(W), P(s2), P(out), n, stream()) == EINVAL
    torch.cuda.synchronize()
    assert pad_is(W.cpu(), 0, SENT) and pad_is(out.cpu(), 0, SENT)


# ====================================================================================================================== block Lanczos
BL_B, BL_K = (1, 8, 15, 16, 17, 32, 40), (1, 127, 128, 129, 300)
# n = 257, 4099: every (b, k); n = 65 573 (the slice count at its cap of 256): the pairs that cross a column group, a basis tile, or neither
BL_CASES = [(n, k, BL_B) for n in (257, 4099) for k in BL_K] + [(65573, 129, (17,)), (65573, 300, (1,)), (65573, 1, (40,))]


@functools.lru_cache(maxsize=2)
def bl_problem(n, dtype):
    g = gen(n)
    return torch.randn(300, n, generator=g, dtype=dtype) / math.sqrt(n), torch.randn(40, n, generator=g, dtype=dtype)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,k,bs", BL_CASES)
def test_block_project(dev, n, k, bs, dtype, variant):
    """gpamd_block_project_f32 / gpamd_block_project_f64: W[c][m] = <R[c], Q[m]>, any b (column groups of 16), any k (tiles of 128 rows)"""
    L = lib()
    fn = L.gpamd_block_project_f64 if dtype == F64 else L.gpamd_block_project_f32
    Qa, Ra = bl_problem(n, dtype)
    ldr, ldq, _ = pc_lds(n, variant)
    Qd = padded(Qa[:k], ldq, dev)
    for b in bs:
        Rd = padded(Ra[:b], ldr, dev)
        nws = int(L.gpamd_precond_coef_workspace_doubles(n, min(b, 16), k))

        def run():
            W, ws = torch.full((b * k + 2,), SENT, device=dev, dtype=F64), torch.full((nws + 2,), SENT, device=dev, dtype=F64)
            ok(fn(P(Qd), ldq, k, P(Rd), ldr, b, n, P(W), P(ws), nws, stream()))
            return dict(W=W.cpu(), ws=ws.cpu())

        got = twice(run)
        within(got["W"][: b * k].view(b, k), S.block_project(Ra[:b], Qa[:k]), 1e-12 * (Ra[:b].double().abs() @ Qa[:k].double().abs().t()), f"W b={b}")
        assert pad_is(got["W"], b * k, SENT) and pad_is(got["ws"], nws, SENT)


BS_B = (1, 15, 16, 17, 32)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n,k,bs", [(n, k, BS_B if n < 65573 else (min(32, b[0]),)) for n, k, b in BL_CASES])
def test_block_subtract(dev, n, k, bs, variant):
    """gpamd_block_subtract_f32: R[c] -= sum_m W[c][m] Q[m], in place, float64 arithmetic, one rounding to float32"""
    L = lib()
    Qa, Ra = bl_problem(n, F32)
    ldr, ldq, _ = pc_lds(n, variant)
    Qd = padded(Qa[:k], ldq, dev)
    for b in bs:
        W = torch.randn(b, k, generator=gen(b * k + n), dtype=F64)
        Wd = W.to(dev)

        def run():
            Rd = padded(Ra[:b], ldr, dev)
            ok(L.gpamd_block_subtract_f32(P(Qd), ldq, k, P(Wd), P(Rd), ldr, b, n, stream()))
            return dict(R=Rd.cpu())

        got = twice(run)["R"]
        ref = S.block_subtract(Qa[:k], W, Ra[:b])
        within(got[:, :n], ref, rounded32(ref, Ra[:b].double().abs() + W.abs() @ Qa[:k].double().abs()), f"R b={b}")
        assert pad_is(got, n, NAN)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", [257, 4099, 65573])
def test_block_transform(dev, n, variant):
    """gpamd_block_transform_f32: R[r] = sum_c M[r][c] R[c] in place; M general (NOT symmetric: a transposed read fails)"""
    L = lib()
    Ra = bl_problem(n, F32)[1]
    ldr = pc_lds(n, variant)[0]
    for b in BS_B if n < 65573 else (17, 32):
        M = torch.randn(b, b, generator=gen(b + n), dtype=F64)
        Md = padded(M.reshape(-1), b * b + 3, dev)

        def run():
            Rd = padded(Ra[:b], ldr, dev)
            ok(L.gpamd_block_transform_f32(P(Md), P(Rd), ldr, b, n, stream()))
            return dict(R=Rd.cpu())

        got = twice(run)["R"]
        ref = S.block_transform(M, Ra[:b])
        within(got[:, :n], ref, rounded32(ref, M.abs() @ Ra[:b].double().abs()), f"R b={b}")
        assert pad_is(got, n, NAN)


def test_block_limits(dev):
    """include/gpamd.h: b <= 32 for subtract / transform (project takes any b)"""
    L, n = lib(), 64
    R, Q, W = torch.full((33, n), 1.0, device=dev), torch.zeros(4, n, device=dev), torch.zeros(33 * 33, device=dev, dtype=F64)
    assert L.gpamd_block_subtract_f32(P(Q), n, 4, P(W), P(R), n, 33, n, stream()) == EINVAL
    assert L.gpamd_block_transform_f32(P(W), P(R), n, 33, n, stream()) == EINVAL
    assert L.gpamd_block_subtract_f32(P(Q), n - 4, 4, P(W), P(R), n, 32, n, stream()) == EINVAL   # ldq < n
    torch.cuda.synchronize()
    assert bool((R == 1.0).all())


# ================================================================================================================== multi-shift MINRES
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n", [3, 1025, 132099])
@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("Q", [1, 3])
def test_msminres_update(dev, Q, t, n, pad):
    """gpamd_msminres_update_f32: d = (v_c - delta d1 - eps d2) / gamma over d2, x += tau d; four distinct coefficients per (q, c): a swapped plane fails"""
    L, g, ld = lib(), gen(n + 10 * t + Q), ru4(n) + pad
    v, d1, d2, x = (torch.randn(*s, generator=g) for s in ((t, n), (Q, t, n), (Q, t, n), (Q, t, n)))
    coef = torch.randn(4, Q, t, generator=g) * 0.25 + torch.tensor([0.5, -1.5, 2.5, -3.5]).view(4, 1, 1)
    vd, d1d, cd = padded(v, ld, dev), padded(d1, ld, dev), coef.to(dev)

    def run():
        d2d, xd = padded(d2, ld, dev), padded(x, ld, dev)
        ok(L.gpamd_msminres_update_f32(P(vd), P(d1d), P(d2d), P(xd), P(cd), Q, t, n, ld, stream()))
        return dict(d=d2d.cpu(), x=xd.cpu())

    got = twice(run)
    dref, xref = S.msminres_update(v, d1, d2, x, coef)
    c = coef.double().unsqueeze(-1)
    dd = elem((v.double().abs().unsqueeze(0) + (c[0] * d1.double()).abs() + (c[1] * d2.double()).abs()) * c[2].abs(), E32)
    within(got["d"][..., :n], dref, dd, "d")
    within(got["x"][..., :n], xref, elem(x.double().abs() + (c[3] * dref).abs(), E32) + c[3].abs() * dd, "x")
    assert pad_is(got["d"], n, NAN) and pad_is(got["x"], n, NAN)
