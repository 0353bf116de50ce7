"""One KISS-GP product W (kron T_i) W^T V on HIP events, split into its three stages -- scatter W^T V, grid-side Toeplitz products, gather W U --
beside the fused exact product ``backend.kv`` of an RBF kernel on the same points: n = 100 000 and 500 000, d = 1, 2, 3, t = 1 and 11 columns, grids
from ``choose_grid_size`` (one grid point per data point).  The preparation of a cloud (cell keys, sort, cell runs: once per cloud and grid) is timed
separately.  python scripts/ski_kv_timing.py [out.json] -> profiles/ski_kv_timing.json"""
import json
import os
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd.utils.grid import choose_grid_size, create_grid  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/ski_kv_timing.json"
assert torch.cuda.is_available(), "timings are taken on the device"
dev = torch.device("cuda:0")
LS = {1: 0.02, 2: 0.08, 3: 0.2}


def timed(fn, reps):
    fn()                                     # warm-up: code objects, library algorithm choices, workspaces
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = []
for n in (100_000, 500_000):
    for d in (1, 2, 3):
        g = torch.Generator().manual_seed(0)
        X = torch.rand(n, d, generator=g).to(dev)
        m = choose_grid_size(X)
        grid = [a.to(dev) for a in create_grid([m] * d, [(0.0, 1.0)] * d)]
        spec = B.SkiGridSpec(grid)
        prep_ms = timed(lambda: B.SkiCloud(X, spec), 3)
        cloud = B.SkiCloud(X, spec)
        cols = [torch.exp(-0.5 * ((a - a[0]) / LS[d]).pow(2)) for a in grid]
        ops = [B.toeplitz_prepare(c) for c in cols]
        plan = B.SkiPlan(cloud, cloud, ops)
        xp = B.prep_points("rbf", X, torch.tensor([LS[d]]), X.mean(0))
        for t in (1, 11):
            vt = torch.randn(t, B.round_up(n, 4), device=dev)
            vt[:, n:] = 0
            ut = B.ski_interp_t(cloud, vt)
            kt = B.kron_matmul(ops, ut).contiguous()
            rec = {"n": n, "d": d, "t": t, "grid": [m] * d, "nodes": spec.nodes, "max_points_per_cell": cloud.max_count, "long_cell_chunks": cloud.nchunks,
                   "prepare_ms": prep_ms,
                   "scatter_ms": timed(lambda: B.ski_interp_t(cloud, vt), 20),
                   "grid_ms": timed(lambda: B.kron_matmul(ops, ut).contiguous(), 20),
                   "gather_ms": timed(lambda: B.ski_interp(cloud, kt), 20),
                   "ski_product_ms": timed(lambda: plan.product(vt), 20),
                   "exact_kv_ms": timed(lambda: B.kv(xp, xp, vt), 3)}
            rec["exact_over_ski"] = rec["exact_kv_ms"] / rec["ski_product_ms"]
            # the two products agree where the grid resolves the lengthscale (a consistency figure, not a test: tests/test_gpu_ski.py has the bounds)
            a, b = plan.product(vt)[:, :n], B.kv(xp, xp, vt)[:, :n]
            rec["max_dev_from_exact_over_max"] = float((a - b).abs().max() / b.abs().max())
            print(rec, flush=True)
            out.append(rec)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(out, open(out_path, "w"), indent=1)
