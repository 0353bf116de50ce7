"""The fused product of the RBF kernel with derivative observations (csrc/kv_rbfgrad.hpp) beside what a Kronecker multitask operator of equal size
costs, in one process on one GPU: at n = 20 000 and 100 000, d = 1 and 3, t = 1 and 11 columns
  fused  K_grad V over vectors of length n (d + 1) (``backend.rbfgrad_kv``: groups of four columns, K regenerated per group);
  rbf    a plain RBF K V with (d + 1) t columns on the same points (``backend.kv``, its own launch policy): the n^2 part of
         ``multitask.kron_matvec`` for d + 1 tasks.
HIP-event medians after a warm-up, the two sides alternating.   python scripts/rbfgrad_kv_timing.py [out.json]   -> profiles/rbfgrad_kv_timing.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else "profiles/rbfgrad_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")


def timed(fns, warm=2, reps=5):
    """Medians (ms) of the callables measured alternately."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(v) for v in ms]


out = {"device": torch.cuda.get_device_name(0), "kv": []}
for n in (20_000, 100_000):
    for d in (1, 3):
        gen = torch.Generator().manual_seed(n + d)
        X = torch.rand(n, d, generator=gen).to(dev)
        ls = torch.full((1, d), 0.1 if d == 1 else 0.3)
        xp = B.prep_points("rbf", X, ls, X.mean(0))
        inv_ls = B.rbfgrad_inv_ls(ls, d, dev)
        for t in (1, 11):
            c = d + 1
            V = torch.zeros(t, B.round_up(n * c, 4), device=dev)
            V[:, : n * c] = torch.randn(t, n * c, generator=torch.Generator().manual_seed(t)).to(dev)
            U = torch.zeros(t * c, B.round_up(n, 4), device=dev)
            U[:, :n] = V[:, : n * c].reshape(t, n, c).permute(0, 2, 1).reshape(t * c, n)
            plan = B.RbfGradPlan(xp, xp, inv_ls, t)
            f_ms, r_ms = timed([lambda: plan.product(V), lambda: B.kv(xp, xp, U)])
            rec = {"n": n, "d": d, "t": t, "fused_rbfgrad_ms": f_ms, "rbf_kv_same_columns_ms": r_ms, "fused_over_rbf": f_ms / r_ms,
                   "pair_columns_per_s": n * n * t / (f_ms * 1e-3)}
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
