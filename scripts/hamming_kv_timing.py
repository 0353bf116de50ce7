"""The Hamming family over packed tokens (GPAMD_HAMMING, csrc/kv_directham.hpp) -- the product K~ V at n sequences of T positions, every prepared
width, beside the rational-quadratic family's product at d = 3 (the family whose radial function it shares) at the same n and column counts in the
same process, on the library's default path for each (``backend.kv`` on prepared clouds: the Hamming family's one kernel; RQ as ``kv_flags``
chooses).  n = 100 000, V = 20, T in {16, 32, 64, 128}, t in {1, 11, 33, 65} columns.  The Hamming family takes 32 (+ 1) columns per launch group:
at t = 65 it generates K twice.  Also recorded: the preparation of one cloud (argmax, packing) and the derivative pass at nine columns.
HIP-event medians of 20 launches after a warm-up, the two families alternating.
    python scripts/hamming_kv_timing.py [n] [out.json]       -> profiles/hamming_kv_timing.json"""
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/hamming_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")
V, ALPHA, BETA = 20, 1.2, 1.5


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


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "vocab_size": V, "alpha": ALPHA, "beta": BETA, "kv": [], "prep": [], "grad": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    X3 = torch.rand(n, 3, generator=gen).to(dev)
    prq = B.prep_points("rq", X3, torch.tensor(0.3), X3.mean(0), 1.5)
    for T in (16, 32, 64, 128):
        tok = torch.randint(0, V, (n, T), generator=gen)
        X = torch.nn.functional.one_hot(tok, V).reshape(n, -1).float().to(dev)
        theta = (V, torch.tensor([ALPHA, BETA]))
        p = B.prep_points("hamming", X, torch.ones(1, 1), None, theta)
        (prep_ms,) = timed([lambda: B.prep_points("hamming", X, torch.ones(1, 1), None, theta)], reps=5)
        out["prep"].append({"T": T, "width_dwords": p.dp, "prepared_bytes": p.xp.numel() * 4, "one_hot_bytes": X.numel() * 4, "prep_ms": prep_ms})
        del X
        for t in (1, 11, 33, 65):
            vt = B.to_probe_major(torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev))
            h_ms, r_ms = timed([lambda: B.kv(p, p, vt), lambda: B.kv(prq, prq, vt)])
            rec = {"T": T, "width_dwords": p.dp, "t": t, "hamming_ms": h_ms, "rq_d3_ms": r_ms, "rq_flags": B.kv_flags(prq, prq, t), "hamming_over_rq_d3": h_ms / r_ms}
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
        lt = B.to_probe_major(torch.randn(n, 9, generator=torch.Generator().manual_seed(1)).to(dev))
        rt = B.to_probe_major(torch.randn(n, 9, generator=torch.Generator().manual_seed(2)).to(dev))
        (g_ms,) = timed([lambda: B.kv_grad_hamming(p, p, lt, rt)], reps=5)
        rec = {"T": T, "width_dwords": p.dp, "t": 9, "hamming_grad_ms": g_ms}
        print(json.dumps(rec), flush=True)
        out["grad"].append(rec)
        del p, vt, lt, rt
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
