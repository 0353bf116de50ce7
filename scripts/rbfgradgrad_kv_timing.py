"""The fused product of the RBF kernel with first- and second-derivative observations (csrc/kv_rbfgradgrad.hpp: 2 d + 1 components per point,
9 d + 1 packed FMAs per pair and column) beside the RBF kernel with first derivatives only (csrc/kv_rbfgrad.hpp: d + 1 components, 3 d + 1 FMAs),
in one process on one GPU, at the same n, d and column count: n = 20 000 and 100 000, d = 1, 3 and 4, t = 1 and 11 columns
  rbfgradgrad  K V over vectors of length n (2 d + 1) (``backend.RbfGradPlan(..., order=2)``);
  rbfgrad      K V over vectors of length n (d + 1) on the same prepared points and lengthscales.
The two operators differ in size -- the second has (2 d + 1)^2 / (d + 1)^2 times the entries per pair -- so the ratio is what second-derivative
data costs at a given n, not a comparison of two implementations of one product.  HIP-event medians after a warm-up, the two sides alternating; the
spread (min .. max over the repetitions) of each side is recorded with it.
    python scripts/rbfgradgrad_kv_timing.py [out.json]   -> profiles/rbfgradgrad_kv_timing.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else "profiles/rbfgradgrad_kv_timing.json"
ORDERS = {"rbfgradgrad": 2, "rbfgrad": 1}
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
    for d in (1, 3, 4):
        gen = torch.Generator().manual_seed(n + d)
        X = torch.rand(n, d, generator=gen).to(dev)
        ls = torch.full((1, d), 0.1 if d == 1 else 0.3)
        inv_ls = B.rbfgrad_inv_ls(ls, d, dev)
        xp = B.prep_points("rbf", X, ls, X.mean(0))
        for t in (1, 11):
            fns = []
            for order in ORDERS.values():
                c = order * d + 1
                V = torch.zeros(t, B.round_up(n * c, 4), device=dev)
                V[:, : n * c] = torch.randn(t, n * c, generator=torch.Generator().manual_seed(t)).to(dev)
                plan = B.RbfGradPlan(xp, xp, inv_ls, t, order=order)
                fns.append(lambda p=plan, v=V: p.product(v))
            res = dict(zip(ORDERS, timed(fns)))
            rec = {"n": n, "d": d, "t": t}
            for name, (med, lo, hi) in res.items():
                c = ORDERS[name] * d + 1
                rec.update({f"{name}_ms": med, f"{name}_min_max_ms": [lo, hi], f"{name}_pair_columns_per_s": n * n * t / (med * 1e-3),
                            f"{name}_block_entries_per_s": n * n * t * c * c / (med * 1e-3)})
            rec["rbfgradgrad_over_rbfgrad"] = res["rbfgradgrad"][0] / res["rbfgrad"][0]
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
