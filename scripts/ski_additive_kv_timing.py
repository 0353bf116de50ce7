"""One additive KISS-GP product W_add blockdiag(T) W_add^T V on HIP events: the fused form (ONE scatter over the concatenation of d one-dimensional
axes, ONE [m, d t] Toeplitz product, ONE gather; csrc/kv_ski_add.hpp) with its scatter and gather alone, beside the same product assembled from d
passes of the one-dimensional entry points ``gpamd_ski_interp_t_f32`` / ``gpamd_ski_interp_f32`` (per input column: scatter, Toeplitz product,
gather, add) -- what the library could do before the additive kernels.  n = 10^5 and 10^6, d = 2, 4, 8, 16, m = 100 nodes per axis, t = 1, 11, 33
columns.  Per figure: one warm-up call, then REPEATS windows of ITERS calls between two events, the two forms alternating; the median window is
reported, with the spread (max - min) / median.  The preparation of the clouds (once per cloud and grid) is timed separately.
python scripts/ski_additive_kv_timing.py [out.json] -> profiles/ski_additive_kv_timing.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd.utils.grid import create_grid  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/ski_additive_kv_timing.json"
assert torch.cuda.is_available(), "timings are taken on the device"
dev = torch.device("cuda:0")
M, LS, REPEATS = 100, 0.1, 7


def windows(fns, iters):
    """Median (and spread) of REPEATS event-timed windows of ``iters`` calls for every function, the functions alternating window by window."""
    for f in fns.values():
        f()                                  # warm-up: code objects, library algorithm choices, workspaces
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in times.items()}


def rows(u):
    """U^T as canonical rows [t, m] (a [1, m] transpose keeps a row stride of 1, which the entry points refuse)."""
    return torch.empty(u.shape[1], u.shape[0], device=u.device, dtype=u.dtype).copy_(u.t())


out = []
axis = create_grid([M], [(0.0, 1.0)])[0].to(dev)
col = torch.exp(-0.5 * ((axis - axis[0]) / LS).pow(2))
op = B.toeplitz_prepare(col)
spec1 = B.SkiGridSpec([axis])
for n in (100_000, 1_000_000):
    for d in (2, 4, 8, 16):
        g = torch.Generator().manual_seed(0)
        X = torch.rand(n, d, generator=g).to(dev)
        spec = B.SkiGridSpec([axis] * d, additive=True)
        cols1 = [X[:, q: q + 1].contiguous() for q in range(d)]
        prep = windows({"fused": lambda: B.SkiCloud(X, spec), "passes": lambda: [B.SkiCloud(c, spec1) for c in cols1]}, 1)
        cloud = B.SkiCloud(X, spec)
        clouds1 = [B.SkiCloud(c, spec1) for c in cols1]
        plan = B.SkiPlan(cloud, cloud, [op])
        for t in (1, 11, 33):
            vt = torch.randn(t, B.round_up(n, 4), device=dev)
            vt[:, n:] = 0
            ut0 = B.ski_interp_t(cloud, vt)
            kt = B.grid_matmul(spec, [op], ut0).contiguous()

            def fused():
                return plan(vt)[0]

            def passes():
                total = None
                for c in clouds1:
                    o = B.ski_interp(c, rows(B.toeplitz_matmul(op, B.ski_interp_t(c, vt).t())))
                    total = o if total is None else total.add_(o)
                return total

            def passes_scatter():
                return [B.ski_interp_t(c, vt) for c in clouds1]

            uts = [rows(B.toeplitz_matmul(op, u.t())) for u in passes_scatter()]

            def passes_gather():
                total = None
                for c, u in zip(clouds1, uts):
                    o = B.ski_interp(c, u)
                    total = o if total is None else total.add_(o)
                return total

            iters = 20 if n * d * t <= 20_000_000 else 5
            r = windows({"fused_product": fused, "passes_product": passes, "fused_scatter": lambda: B.ski_interp_t(cloud, vt),
                         "passes_scatter": passes_scatter, "fused_gather": lambda: B.ski_interp(cloud, kt), "passes_gather": passes_gather,
                         "fused_grid": lambda: B.grid_matmul(spec, [op], ut0).contiguous()}, iters)
            a, b = fused()[:, :n], passes()[:, :n]
            rec = {"n": n, "d": d, "t": t, "m": M, "nodes": spec.nodes, "long_cell_chunks": cloud.nchunks, "windows": REPEATS, "calls_per_window": iters,
                   "prepare_fused_ms": prep["fused"][0], "prepare_passes_ms": prep["passes"][0]}
            for k, (med, spread) in r.items():
                rec[k + "_ms"] = med
                rec[k + "_spread"] = spread
            for k in ("product", "scatter", "gather"):
                rec[f"passes_over_fused_{k}"] = rec[f"passes_{k}_ms"] / rec[f"fused_{k}_ms"]
            rec["max_dev_fused_from_passes_over_max"] = float((a - b).abs().max() / b.abs().max())   # (summation orders differ: last bits)
            print(rec, flush=True)
            out.append(rec)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(out, open(out_path, "w"), indent=1)
