"""The linear model of coregionalisation (csrc/kv_lcm.hpp) -- the product (sum_q theta_q K_q (x) B_q) V on the fused multi-member kernel, pre-pass
included, beside the same product assembled from the single-family form: sum over the members of ``multitask.kron_matvec`` on per-member prepared
clouds, host adds included.  n = 100 000, d = 3, Q in {2, 3, 4} (RBF, Matern 3/2, 5/2, 1/2 in turn), T in {2, 4}, 1 and 11 probes.  HIP-event
medians of 20 launches after a warm-up, the two forms alternating.
    python scripts/lcm_kv_timing.py [n] [out.json]       -> profiles/lcm_kv_timing.json"""
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd.multitask import kron_matvec  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/lcm_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")
KINDS = ("rbf", "matern32", "matern52", "matern12")


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


out = {"n": n, "d": 3, "device": torch.cuda.get_device_name(0), "reps": 20, "kv": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    X = torch.rand(n, 3, generator=gen).to(dev)
    shift = X.mean(0)
    xc = B.lcm_points(X, shift)
    for Q in (2, 3, 4):
        ls = [torch.tensor([0.2 + 0.1 * q]) for q in range(Q)]
        preps = [B.prep_points(KINDS[q], X, ls[q], shift) for q in range(Q)]
        for T in (2, 4):
            bs = []
            for q in range(Q):
                f = torch.randn(T, 1, generator=gen)
                bs.append((f @ f.t() + torch.diag(torch.rand(T, generator=gen) + 0.2)).to(dev))
            block = B.lcm_block(KINDS[:Q], ls, bs, 3)
            for t in (1, 11):
                vt = B.to_probe_major(torch.randn(n * T, t, generator=torch.Generator().manual_seed(t)).to(dev))
                plan = B.LcmPlan(xc, xc, block, 3, T, t)

                def base():
                    acc = kron_matvec(preps[0], preps[0], bs[0], vt)
                    for q in range(1, Q):
                        acc = acc + kron_matvec(preps[q], preps[q], bs[q], vt)
                    return acc

                f_ms, b_ms = timed([lambda: plan.product(vt), base])
                dev_rel = float((plan.product(vt)[:, : n * T] - base()[:, : n * T]).abs().max() / base()[:, : n * T].abs().max())
                rec = {"Q": Q, "T": T, "probes": t, "fused_ms": f_ms, "members_ms": b_ms, "members_over_fused": b_ms / f_ms, "S": plan.S, "max_rel_dev": dev_rel}
                print(json.dumps(rec), flush=True)
                out["kv"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
