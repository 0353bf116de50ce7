"""Fused float64 K*V for 17 .. 512 input dimensions (csrc/kv_f64_wide.hpp) against the row-block x DGEMM path (backend.FORCE_CHUNKED) in the same
run, the two alternating.  Usage: python scripts/f64_wide_kv_timing.py [--n 20000] [--out profiles/f64_wide_kv_timing.json]

Per shape: median host-clock time of a product that ends in a device synchronise (after a warm-up of both paths), the largest deviation between the
two results relative to the largest entry, and the share of the float64 matrix-pipe peak that the Gram MFMAs ALONE account for: n m dp multiply-adds
over the fused time, against CUs x 4 SIMDs x 16 multiply-adds per cycle x 2.4 GHz (v_mfma_f64_16x16x4_f64: 1024 multiply-adds in 64 cycles)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20000, help="points per cloud: small enough for the row-block side (seconds per product at d = 512)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default="profiles/f64_wide_kv_timing.json")
args = ap.parse_args()

dev = torch.device("cuda:0")
peak_fma = torch.cuda.get_device_properties(dev).multi_processor_count * 4 * 16 * 2.4e9
n = args.n


def timed(xp, vt, force, calls):
    B.FORCE_CHUNKED = force
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = B.kv(xp, xp, vt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls, out
    finally:
        B.FORCE_CHUNKED = False


result = dict(n=n, m=n, device=torch.cuda.get_device_name(dev), peak_f64_mfma_fma_per_s=peak_fma, rounds=args.rounds, shapes=[])
for d in (20, 40, 90, 256, 512):
    X = torch.rand(n, d, device=dev, dtype=torch.float64)
    for kind in ("rbf", "matern52"):
        xp = B.prep_points(kind, X, torch.tensor(0.4 * math.sqrt(d), dtype=torch.float64), X.mean(0))
        assert B.fused_f64(xp, xp)
        for t in (1, 11, 65):
            vt = torch.randn(t, B.round_up(n, 4), device=dev, dtype=torch.float64)
            w_f, o_f = timed(xp, vt, False, 1)          # warm-up of both paths; also the comparison of their results
            w_r, o_r = timed(xp, vt, True, 1)
            dev_rel = float((o_f[:, :n] - o_r[:, :n]).abs().max() / o_r[:, :n].abs().max())
            calls_f = max(1, min(50, int(0.2 / max(w_f, 1e-5))))
            tf, tr = [], []
            for _ in range(args.rounds):
                tf.append(timed(xp, vt, False, calls_f)[0])
                tr.append(timed(xp, vt, True, 1)[0])
            f_ms, r_ms = 1e3 * statistics.median(tf), 1e3 * statistics.median(tr)
            rec = dict(kind=kind, d=d, dp=xp.dp, t=t, fused_ms=f_ms, fused_ms_all=[1e3 * v for v in tf], rowblock_ms=r_ms,
                       rowblock_ms_all=[1e3 * v for v in tr], speedup=r_ms / f_ms, max_rel_deviation=dev_rel,
                       gram_mfma_peak_fraction=n * n * xp.dp / (f_ms * 1e-3) / peak_fma)
            print(json.dumps(rec), flush=True)
            result["shapes"].append(rec)
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            json.dump(result, open(args.out, "w"), indent=1)
