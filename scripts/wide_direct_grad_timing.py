"""Timing of the fused wide bilinear derivative by direct differences (csrc/kv_wide_direct_grad.hpp) beside the row-block route it replaces and beside
the forward product, on one device in one run.

For n = 100 000 points, d in {40, 90, 256, 512}, t in {11, 65} columns, RBF (a cloud 20 lengthscales from the common origin: beyond the norm rule of the
Gram form) and Matern-1/2, with W = L^T R of positive-mean vector blocks:
  iso_ms, ard_ms, gz_ms   backend.kv_grad_wide_direct in the single-lengthscale mode, the per-dimension mode, and per dimension + Gz1: median of
                          ``--reps`` calls after one warm-up call;
  forward_ms              K(x, x) @ V with the same t on the direct-difference kernel (backend.WideDirectPlan.product through backend.kv), the same way;
  generic_ms              backend.kv_grad_generic for the same operands (dense row blocks of W from a library GEMM, float64 sums; what hyper_grads runs
                          with backend.WIDE_KV = False): ONE call, no warm-up -- it takes seconds at this n.  It has no Gz1 at these dimensions, so only
                          iso_ms and ard_ms compare with it;
  max_rel_dev             the largest relative deviation of the fused per-dimension sums from the generic ones.
The fused modes of every shape are timed first; the generic route follows shape by shape until ``--budget-s`` is used up (``cut_short`` then says so).
Every time is a host clock around calls that end in a device synchronise.  Results go to the JSON file after every shape.
Usage: python scripts/wide_direct_grad_timing.py [--n 100000] [--reps 3] [--out profiles/wide_direct_grad_timing.json] [--budget-s 420]"""
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
    ap.add_argument("--out", default="profiles/wide_direct_grad_timing.json")
    ap.add_argument("--budget-s", type=float, default=420.0)
    a = ap.parse_args()
    from gpytorch_amd import backend as B

    if not torch.cuda.is_available():
        raise SystemExit("wide_direct_grad_timing: needs a ROCm device")
    dev = torch.device("cuda:0")
    res = {"n": a.n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": []}
    start = time.perf_counter()

    def operands(kind, d, t):
        g0 = torch.Generator().manual_seed(1000 * d + t)
        X = torch.rand(a.n, d, generator=g0).to(dev)
        ls = math.sqrt(d) / 4
        xp = B.prep_points(kind, X, torch.tensor(ls), X.mean(0) - (0.0 if kind == "matern12" else 20.0 * ls / math.sqrt(d)))
        lt = (1 + 0.3 * torch.randn(t, a.n, generator=g0)).to(dev)
        rt = lt + 0.5 * torch.randn(t, a.n, generator=g0).to(dev)
        return xp, lt, rt

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    shapes = [(kind, t, d) for kind in ("rbf", "matern12") for t in (11, 65) for d in (40, 90, 256, 512)]
    for kind, t, d in shapes:
        xp, lt, rt = operands(kind, d, t)
        assert B.wide_direct_f32(xp, xp)
        row = {"kind": kind, "d": d, "t": t}
        row["iso_ms"] = timed(lambda: B.kv_grad_wide_direct(xp, xp, lt, rt, iso=True), a.reps)
        row["ard_ms"] = timed(lambda: B.kv_grad_wide_direct(xp, xp, lt, rt), a.reps)
        row["gz_ms"] = timed(lambda: B.kv_grad_wide_direct(xp, xp, lt, rt, want_gz1=True), a.reps)
        row["forward_ms"] = timed(lambda: B.kv(xp, xp, rt), a.reps)
        res["rows"].append(row)
        print(row, flush=True)
        save()
        del xp, lt, rt
    for row in res["rows"]:
        if time.perf_counter() - start > a.budget_s:
            res["cut_short"] = True
            break
        xp, lt, rt = operands(row["kind"], row["d"], row["t"])
        fused = B.kv_grad_wide_direct(xp, xp, lt, rt)[0][: 1 + row["d"]].double()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = B.kv_grad_generic(xp, xp, lt, rt)[: 1 + row["d"]]
        torch.cuda.synchronize()
        row["generic_ms"] = 1e3 * (time.perf_counter() - t0)
        row["max_rel_dev"] = float(((fused - ref).abs() / ref.abs()).max())
        print(row, flush=True)
        save()
        del xp, lt, rt
    save()


if __name__ == "__main__":
    main()
