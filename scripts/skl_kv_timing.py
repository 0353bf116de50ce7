"""The symmetrized-KL family over Gaussian inputs (GPAMD_SKL, csrc/kv_directskl.hpp) beside the Gibbs family (csrc/kv_directgibbs.hpp) -- the same
kernel body, one 32-column tile, a lazy functor, one transcendental fewer per pair -- at the Gibbs width nearest to the SKL width (SKL 4 / 12 / 20 for
d = 1 / 3 / 6 against Gibbs 4 / 8 / 8 at its d = 1 / 3 / 6), in one process on one GPU, through the kernel API (``op @ V`` without autograd: point
preparation + product, as a solver iteration pays for it).  n = 100 000, t in {1, 11, 33, 65} columns; both families take 32 (+ 1) columns per launch
group, so 65 columns generate K twice.  Then one derivative pass (``backend.kv_grad_skl``: G0, G1 and the gradient of every point's mean and variance)
at t = 11 beside the Gibbs pass.  HIP-event medians of 20 launches after a warm-up, the operators alternating.
    python scripts/skl_kv_timing.py [n] [out.json]       -> profiles/skl_kv_timing.json"""
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402
from gpytorch_amd import backend as B  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/skl_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")


class Field(torch.nn.Module):
    """A fixed smooth lengthscale field, l(x) in [0.08 d, 0.32 d] (scripts/gibbs_kv_timing.py)."""

    def forward(self, x):
        return x.shape[-1] * (0.2 + 0.12 * torch.sin(3.0 * x.sum(-1, keepdim=True) + 0.5))


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


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "kv": [], "grad": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    for d in (1, 3, 6):
        mu = torch.rand(n, d, generator=gen)
        Z = torch.cat([mu, -3.0 + 2.0 * torch.rand(n, d, generator=gen)], -1).to(dev)
        skl, gib = g.kernels.GaussianSymmetrizedKLKernel().to(dev), g.kernels.GibbsKernel(Field()).to(dev)
        skl.lengthscale = float(d)
        ops = [skl(Z), gib(mu.to(dev))]
        assert [o.spec.kind for o in ops] == ["skl", "gibbs"]
        widths = [o.prepared()[0].dp for o in ops]
        for t in (1, 11, 33, 65):
            V = torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev)
            s_ms, g_ms = timed([lambda: ops[0] @ V, lambda: ops[1] @ V])
            rec = {"d": d, "t": t, "skl_width": widths[0], "gibbs_width": widths[1], "skl_ms": s_ms, "gibbs_ms": g_ms, "skl_over_gibbs": s_ms / g_ms}
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
        t = 11
        lt, rt = (B.to_probe_major(torch.randn(n, t, generator=torch.Generator().manual_seed(k)).to(dev)) for k in (1, 2))
        (ps, _), (pg, _) = (o.prepared() for o in ops)
        s_ms, g_ms = timed([lambda: B.kv_grad_skl(ps, ps, lt, rt), lambda: B.kv_grad_gibbs(pg, pg, lt, rt)])
        rec = {"d": d, "t": t, "skl_grad_ms": s_ms, "gibbs_grad_ms": g_ms, "skl_over_gibbs": s_ms / g_ms}
        print(json.dumps(rec), flush=True)
        out["grad"].append(rec)
        del Z, ops, V, lt, rt
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
