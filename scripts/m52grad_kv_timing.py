"""The fused product of the Matern-5/2 kernel with derivative observations beside the RBF one (both csrc/kv_rbfgrad.hpp: the same kernel body, three
radial factors from one sqrt and one exp2 against one factor from one exp2), in one process on one GPU: at n = 20 000 and 100 000, d = 1 and 3,
t = 1 and 11 columns
  m52grad  K_grad V over vectors of length n (d + 1) on the Matern-5/2-prepared points (``backend.rbfgrad_kv``: the family is the points');
  rbfgrad  the same product on the RBF-prepared points of the same cloud and lengthscales.
HIP-event medians after a warm-up, the two sides alternating; the spread (min .. max over the repetitions) of each side is recorded with it.
    python scripts/m52grad_kv_timing.py [out.json]   -> profiles/m52grad_kv_timing.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else "profiles/m52grad_kv_timing.json"
FAMILIES = ("matern52", "rbf")
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")


def timed(fns, warm=2, reps=7):
    """(median, min, max) in ms of the callables measured alternately."""
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
    return [(statistics.median(v), min(v), max(v)) for v in ms]


out = {"device": torch.cuda.get_device_name(0), "kv": []}
for n in (20_000, 100_000):
    for d in (1, 3):
        gen = torch.Generator().manual_seed(n + d)
        X = torch.rand(n, d, generator=gen).to(dev)
        ls = torch.full((1, d), 0.1 if d == 1 else 0.3)
        inv_ls = B.rbfgrad_inv_ls(ls, d, dev)
        preps = {f: B.prep_points(f, X, ls, X.mean(0)) for f in FAMILIES}
        for t in (1, 11):
            c = d + 1
            V = torch.zeros(t, B.round_up(n * c, 4), device=dev)
            V[:, : n * c] = torch.randn(t, n * c, generator=torch.Generator().manual_seed(t)).to(dev)
            plans = [B.RbfGradPlan(preps[f], preps[f], inv_ls, t) for f in FAMILIES]
            res = dict(zip(FAMILIES, timed([(lambda p=p: p.product(V)) for p in plans])))
            rec = {"n": n, "d": d, "t": t}
            for f, (med, lo, hi) in res.items():
                rec.update({f"{B.GRAD_FAMILIES[f]}_ms": med, f"{B.GRAD_FAMILIES[f]}_min_max_ms": [lo, hi],
                            f"{B.GRAD_FAMILIES[f]}_pair_columns_per_s": n * n * t / (med * 1e-3)})
            rec["m52grad_over_rbfgrad"] = res["matern52"][0] / res["rbf"][0]
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
