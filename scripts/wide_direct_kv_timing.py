"""Timing of the fused wide product by direct differences (csrc/kv_wide_direct.hpp) beside the row-block path it replaces and beside the Gram-form
wide kernel, on one device in one run.

For n = 100 000 points, d in {40, 90, 256, 512}, t in {1, 11, 65} columns, an RBF cloud beyond the norm rule (U[0, 1]^d, lengthscale sqrt(d) / 4, the
common origin 20 lengthscales from the cloud: max |z|^2 > 32) and Matern 1/2 on the same cloud centred:
  direct_ms    K(x, x) @ V on the direct-difference kernel (backend.WideDirectPlan.product), median of ``--reps`` calls after one warm-up call;
  chunked_ms   the same product with backend.WIDE_KV = False (dense row blocks of K x library GEMM: the route before this kernel): ONE call, no
               warm-up -- a call takes seconds at this n, against which first-launch effects (milliseconds) do not count;
  wide_ms      the Gram-form wide kernel (backend.WidePlan.product) on the RBF cloud of the same n, d, t centred on its mean, which it admits.
Every time is a host clock around calls that end in a device synchronise.  Shapes run in the order d, kind, t; results go to the JSON file after
every shape, so a run that ends at ``--budget-s`` keeps what it measured and says ``cut_short``.
Usage: python scripts/wide_direct_kv_timing.py [--n 100000] [--reps 3] [--out profiles/wide_direct_kv_timing.json] [--budget-s 420]"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scripts.wide_kv_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/wide_direct_kv_timing.json")
    ap.add_argument("--budget-s", type=float, default=420.0)
    a = ap.parse_args()
    from gpytorch_amd import backend as B

    if not torch.cuda.is_available():
        raise SystemExit("wide_direct_kv_timing: needs a ROCm device")
    dev = torch.device("cuda:0")
    g0 = torch.Generator().manual_seed(0)
    res = {"n": a.n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": []}
    start = time.perf_counter()
    vts = {t: B.to_probe_major(torch.randn(a.n, t, generator=g0).to(dev)) for t in (1, 11, 65)}
    for d in (40, 90, 256, 512):
        X = torch.rand(a.n, d, generator=g0).to(dev)
        ls, mean = torch.tensor(math.sqrt(d) / 4), X.mean(0)
        near = B.prep_points("rbf", X, ls, mean)
        clouds = {"rbf": B.prep_points("rbf", X, ls, mean - 20.0 * float(ls) / math.sqrt(d)), "matern12": B.prep_points("matern12", X, ls, mean)}
        assert B.wide_f32(near, near)
        for kind, xp in clouds.items():
            assert B.wide_direct_f32(xp, xp) and not B.wide_f32(xp, xp)
            for t, vt in vts.items():
                if time.perf_counter() - start > a.budget_s:
                    res["cut_short"] = True
                    break
                direct = timed(lambda: B.kv(xp, xp, vt), a.reps)
                od = B.kv(xp, xp, vt)[:, : a.n].clone()
                wide = timed(lambda: B.kv(near, near, vt), a.reps)
                B.WIDE_KV = False
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    oc = B.kv(xp, xp, vt)[:, : a.n]
                    torch.cuda.synchronize()
                    chunked = 1e3 * (time.perf_counter() - t0)
                finally:
                    B.WIDE_KV = True
                dev_rel = float((od - oc).abs().max() / oc.abs().max())
                res["rows"].append({"kind": kind, "d": d, "t": t, "zmax2": xp.zmax2, "direct_ms": direct, "chunked_ms": chunked, "wide_ms": wide,
                                    "max_rel_dev_direct_vs_chunked": dev_rel})
                print(res["rows"][-1], flush=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                del od, oc
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
