"""Times the fused bilinear derivative (backward of one MLL evaluation) at the bench shape against one K*V of equal flops:
Gram-form kernel (kv_grad2, single lengthscale / ARD / ARD + input gradients) vs the direct-difference kernel (kv_grad).
Usage: python scripts/grad_timing.py [tag] [n] [t] [families]  -> grad_timing_<tag>.json in the output directory of the timing scripts"""
# With a fourth argument, a comma-separated list out of single,prod,add,sm,ng,gibbs, it times ONLY the direct derivative call of those families' kernels
# (csrc/kv_grad.hpp's W tile with each family's functor), one shape each -- the family's case in its own timing script (product_kv_timing.py,
# additive_kv_timing.py, sm_kv_timing.py, newton_girard_kv_timing.py, gibbs_kv_timing.py; t = 11 columns there, [t] here for the single family) -- at n
# points: the median of 7 HIP-event timings after a warm-up.  For an A/B of two builds run it once per build (GPAMD_LIBRARY) and alternate.
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "x"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
t = int(sys.argv[3]) if len(sys.argv) > 3 else 65
dev = torch.device("cuda:0")


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def family_cases():
    """name -> the direct derivative call of one kernel of csrc/kv_grad.hpp / kv_grad_ng.hpp / kv_grad_gibbs.hpp."""
    gen = torch.Generator().manual_seed(0)
    ld = B.round_up(n, 4)

    def lr(tt):
        return torch.randn(tt, ld, generator=gen).to(dev), torch.randn(tt, ld, generator=gen).to(dev)

    def single():
        X = torch.rand(n, 3, generator=gen).to(dev)
        xp = B.prep_points("rbf", X, torch.tensor(0.25), X.mean(0))
        L, R = lr(t)
        return lambda: B.kv_grad(xp, xp, L, R, iso=False)

    def prod():   # matern52(1) x rbf(2), canonical order: the RBF columns first
        X = torch.rand(n, 3, generator=gen).to(dev)
        xp = B.prep_points("prod", X, torch.tensor([0.5, 0.5, 0.3]), X.mean(0), B.prod_code(0, 3, 2))
        L, R = lr(11)
        return lambda: B.kv_grad(xp, xp, L, R, iso=False)

    def add():
        X = torch.rand(n, 4, generator=gen).to(dev)
        xp = B.prep_points("add", X, 0.2 + 0.15 * torch.rand(1, 4, generator=gen), X.mean(0), B.add_code("matern52"))
        L, R = lr(11)
        return lambda: B.kv_grad(xp, xp, L, R, iso=False)

    def sm():
        X = torch.rand(n, 1, generator=gen).to(dev)
        w, mu, sigma = torch.tensor([0.5, 0.8, 0.3, 0.6]), torch.tensor([0.7, 1.9, 3.1, 5.2]).reshape(4, 1), torch.tensor([0.9, 1.2, 1.0, 1.4]).reshape(4, 1)
        xp = B.prep_points("sm", X, torch.ones(1, 1), X.mean(0), B.sm_theta(w, mu, sigma).to(dev))
        L, R = lr(11)
        return lambda: B.kv_grad_sm(xp, xp, L, R)

    def ng():
        X = torch.rand(n, 4, generator=gen).to(dev)
        sigma = (0.2 + torch.rand(3, generator=gen)).to(dev)
        xp = B.prep_points("ng", X, 0.2 + 0.15 * torch.rand(1, 4, generator=gen), X.mean(0), (B.add_code("matern52"), sigma))
        L, R = lr(11)
        return lambda: B.kv_grad_ng(xp, xp, L, R)

    def gibbs():
        X = torch.rand(n, 3, generator=gen)
        z = torch.cat([X, 0.15 + 0.75 * torch.rand(n, 1, generator=gen)], -1).to(dev)
        xp = B.prep_points("gibbs", z, torch.ones(1, 1, device=dev), torch.cat([z[:, :3].mean(0), z.new_zeros(1)]))
        L, R = lr(11)
        return lambda: B.kv_grad_gibbs(xp, xp, L, R)

    return {"single": single, "prod": prod, "add": add, "sm": sm, "ng": ng, "gibbs": gibbs}


if len(sys.argv) > 4:
    cases, res = family_cases(), {}
    for name in sys.argv[4].split(","):
        fn = cases[name]()
        res[name] = statistics.median(timed(fn, reps=1) for _ in range(7))
        print(name, res[name], flush=True)
    out = {"n": n, "t_single": t, "t_family": 11, "library": os.environ.get("GPAMD_LIBRARY", "csrc/libgpamd.so"), "ms": res}
    SHAPES = ()   # the families only; the record is written below
else:
    out = []
    SHAPES = (("rbf", 3, 0.25), ("matern52", 10, 0.8))
for kind, d, ls in SHAPES:
    X = torch.rand(n, d, generator=torch.Generator().manual_seed(0)).to(dev)
    xp = B.prep_points(kind, X, torch.tensor(ls), X.mean(0))
    lt = torch.randn(t, B.round_up(n, 4), device=dev)
    rt = torch.randn(t, B.round_up(n, 4), device=dev)
    flop = 2.0 * n * n * t
    rec = dict(kind=kind, n=n, d=d, t=t)
    rec["kv_ms"] = timed(lambda: B.kv(xp, xp, rt))
    rec["grad_direct_iso_ms"] = timed(lambda: B.kv_grad(xp, xp, lt, rt, iso=True))
    rec["grad_direct_ard_ms"] = timed(lambda: B.kv_grad(xp, xp, lt, rt, iso=False))
    for split in (False, True):   # W = L^T R on the fp32 MFMAs / on hi-lo split f16 operands (kv_grad2.hpp WSPLIT)
        B.SPLIT_CONTRACTION = split
        sfx = "_split" if split else ""
        rec["grad2_iso%s_ms" % sfx] = timed(lambda: B.kv_grad2(xp, xp, lt, rt, iso=True))
        rec["grad2_ard%s_ms" % sfx] = timed(lambda: B.kv_grad2(xp, xp, lt, rt, iso=False))
        rec["grad2_ard_xgrad%s_ms" % sfx] = timed(lambda: B.kv_grad2(xp, xp, lt, rt, iso=False, want_gz1=True))
        # accuracy on NON-cancelling vectors (|randn|): random-sign vectors make the n^2-term sums cancel by ~1e4, which turns the 2^-22
        # operand precision of either contraction into an apparent 1e-3 "deviation" between any two summation orders
        la, ra = lt.abs(), rt.abs()
        a = B.kv_grad(xp, xp, la, ra, iso=False)
        b, _ = B.kv_grad2(xp, xp, la, ra, iso=False)
        rec["max_rel_dev_vs_direct" + sfx] = float(((a - b[: a.numel()]).abs() / a.abs().clamp_min(1e-30))[: 1 + d].max())
        b0, _ = B.kv_grad2(xp, xp, la, ra, iso=True)
        rec["iso_rel_dev_vs_direct" + sfx] = float(abs(float(a[1 : 1 + d].sum()) - float(b0[1])) / abs(float(a[1 : 1 + d].sum())))
    B.SPLIT_CONTRACTION = None
    for k in list(rec):
        if k.endswith("_ms"):
            rec[k.replace("_ms", "_tflops")] = flop / rec[k] / 1e9
    print(rec, flush=True)
    out.append(rec)
os.makedirs("gpurun_out", exist_ok=True)
json.dump(out, open(f"gpurun_out/grad_timing_{tag}.json", "w"), indent=1)
