"""Timing of the fused wide product (csrc/kv_wide.hpp) beside the row-block path it replaces, on one device in one run.

For n = 100 000 points, d in {40, 64, 90, 128, 256, 385, 512}, t in {1, 11, 65} columns, RBF and Matern-5/2:
  wide_ms      K(x, x) @ V on the wide kernel (backend.WidePlan.product), median of ``--reps`` calls after one warm-up call;
  chunked_ms   the same product with backend.WIDE_KV = False (dense row blocks of K x library GEMM: the route before the wide kernel): ONE call,
               no warm-up -- a call takes 3 - 30 s at this n, against which first-launch effects (milliseconds) do not count, and the grid has 42 shapes;
  split_ms     the split pre-pass of the cloud (gpamd_wide_split_f32), timed separately -- it runs once per prepared cloud;
  fused32_ms   the d = 32 fused product of the same n and t (the nearest shape the register-resident kernels serve).
Every time is a host clock around calls that end in a device synchronise.  Results go to the JSON file after every shape, so a run that is cut short
keeps what it measured.
Usage: python scripts/wide_kv_timing.py [--n 100000] [--reps 3] [--out profiles/wide_kv_timing.json] [--budget-s 420]"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/wide_kv_timing.json")
    ap.add_argument("--budget-s", type=float, default=420.0)
    a = ap.parse_args()
    from gpytorch_amd import backend as B

    if not torch.cuda.is_available():
        raise SystemExit("wide_kv_timing: needs a ROCm device")
    dev = torch.device("cuda:0")
    g0 = torch.Generator().manual_seed(0)
    res = {"n": a.n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": []}
    start = time.perf_counter()

    def cloud(kind, d):
        X = torch.rand(a.n, d, generator=g0).to(dev)
        return B.prep_points(kind, X, torch.tensor(math.sqrt(d) / 4), X.mean(0))

    for kind in ("rbf", "matern52"):
        x32 = cloud(kind, 32)
        for t in (1, 11, 65):
            vt = B.to_probe_major(torch.randn(a.n, t, generator=g0).to(dev))
            fused32 = timed(lambda: B.kv(x32, x32, vt), a.reps)
            for d in (40, 64, 90, 128, 256, 385, 512):
                if time.perf_counter() - start > a.budget_s:
                    res["cut_short"] = True
                    break
                xp = cloud(kind, d)
                B.wide_image(xp)   # (warm-up of the pre-pass)
                torch.cuda.synchronize()
                xp._wide = None
                t0 = time.perf_counter()
                B.wide_image(xp)
                torch.cuda.synchronize()
                split = 1e3 * (time.perf_counter() - t0)
                assert B.wide_f32(xp, xp)
                wide = timed(lambda: B.kv(xp, xp, vt), a.reps)
                ow = B.kv(xp, xp, vt)[:, : a.n].clone()
                B.WIDE_KV = False
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    oc = B.kv(xp, xp, vt)[:, : a.n]
                    torch.cuda.synchronize()
                    chunked = 1e3 * (time.perf_counter() - t0)
                finally:
                    B.WIDE_KV = True
                dev_rel = float((ow - oc).abs().max() / oc.abs().max())
                res["rows"].append({"kind": kind, "d": d, "t": t, "wide_ms": wide, "chunked_ms": chunked, "split_ms": split, "fused32_ms": fused32,
                                    "max_rel_dev_wide_vs_chunked": dev_rel})
                print(res["rows"][-1], flush=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                del xp, ow, oc
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
