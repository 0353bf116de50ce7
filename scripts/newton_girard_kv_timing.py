"""The Newton-Girard additive family (GPAMD_NG, csrc/kv_directng.hpp) beside the first-order additive family (KIND_ADD, csrc/kv_directadd.hpp) at the
same base family, d and column count, in one process on one GPU, through the kernel API (``op @ V`` without autograd: point preparation + product, as
a solver iteration pays for it).  Both generate the same d one-dimensional covariances per pair; the polynomial on top is what the ratio prices.
n = 100 000, d in {4, 8}, degree caps 3 and d (max_degree = 3 and d), t in {1, 11, 65} columns, RBF and Matern-5/2.  HIP-event medians of 20 launches
after a warm-up, the three operators alternating.
    python scripts/newton_girard_kv_timing.py [n] [out.json]       -> profiles/newton_girard_kv_timing.json"""
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/newton_girard_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")


def timed(fns, warm=3, reps=20):
    """Medians (ms) of the callables, measured alternately."""
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


def base_kernel(kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=2.5, **kw)


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "kv": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    for kind in ("rbf", "matern52"):
        for d in (4, 8):
            X = torch.rand(n, d, generator=gen).to(dev)
            ls = 0.2 + 0.15 * torch.rand(1, d, generator=gen)
            add = g.kernels.AdditiveStructureKernel(base_kernel(kind, ard_num_dims=d), num_dims=d).to(dev)
            add.base_kernel.lengthscale = ls
            ngs = []
            for r in (3, d):
                k = g.kernels.NewtonGirardAdditiveKernel(base_kernel(kind, ard_num_dims=d), num_dims=d, max_degree=r).to(dev)
                k.base_kernel.lengthscale = ls
                ngs.append(k)
            ops = [add(X), ngs[0](X), ngs[1](X)]
            assert ops[0].spec.kind == "add" and ops[1].spec.kind == ops[2].spec.kind == "ng"
            for t in (1, 11, 65):
                V = torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev)
                a_ms, c3_ms, cd_ms = timed([lambda: ops[0] @ V, lambda: ops[1] @ V, lambda: ops[2] @ V])
                rec = {"base": kind, "d": d, "t": t, "additive_ms": a_ms, "ng_cap3_ms": c3_ms, "ng_capd_ms": cd_ms,
                       "cap3_over_additive": c3_ms / a_ms, "capd_over_additive": cd_ms / a_ms}
                print(json.dumps(rec), flush=True)
                out["kv"].append(rec)
            del X, ops, V
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
