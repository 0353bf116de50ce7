"""The Gibbs family (GPAMD_GIBBS, csrc/kv_directgibbs.hpp) beside the RBF and the Matern-5/2 single-family products on the SAME path -- direct differences
on the packed-f32 pipe, contraction of hi/lo-split operands on the f16 matrix pipe (csrc/kv_directh.hpp; ``backend.FORCE_KV_FLAGS`` keeps the two
stationary families off their Gram-form kernels and, below five columns, off the few-column kernels) -- in one process on one GPU, through the kernel
API (``op @ V`` without autograd: point preparation + product, as a solver iteration pays for it).  n = 100 000, d in {1, 3}, t in {1, 11, 65}
columns.  The stationary families take up to 64 (+ 1) columns per launch group, the Gibbs family 32 (+ 1): at t = 65 it generates K twice.
HIP-event medians of 20 launches after a warm-up, the three operators alternating.
    python scripts/gibbs_kv_timing.py [n] [out.json]       -> profiles/gibbs_kv_timing.json"""
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
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/gibbs_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")


class Field(torch.nn.Module):
    """A fixed smooth lengthscale field, l(x) in [0.08 d, 0.32 d]."""

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


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "path": "direct differences + split contraction (KV_SPLIT | KV_SPLIT_FEW)", "kv": []}
gen = torch.Generator().manual_seed(0)
B.FORCE_KV_FLAGS = B.KV_SPLIT | B.KV_SPLIT_FEW
with torch.no_grad():
    for d in (1, 3):
        X = torch.rand(n, d, generator=gen).to(dev)
        rbf, m52, gib = g.kernels.RBFKernel().to(dev), g.kernels.MaternKernel(nu=2.5).to(dev), g.kernels.GibbsKernel(Field()).to(dev)
        rbf.lengthscale = m52.lengthscale = 0.2 * d
        ops = [rbf(X), m52(X), gib(X)]
        assert [o.spec.kind for o in ops] == ["rbf", "matern52", "gibbs"]
        for t in (1, 11, 65):
            V = torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev)
            for o in ops[:2]:
                p = o.prepared()[0]
                assert B.kv_flags(p, p, t) == B.FORCE_KV_FLAGS
            r_ms, m_ms, g_ms = timed([lambda: ops[0] @ V, lambda: ops[1] @ V, lambda: ops[2] @ V])
            rec = {"d": d, "t": t, "rbf_ms": r_ms, "matern52_ms": m_ms, "gibbs_ms": g_ms, "gibbs_over_rbf": g_ms / r_ms, "gibbs_over_matern52": g_ms / m_ms}
            print(json.dumps(rec), flush=True)
            out["kv"].append(rec)
        del X, ops, V
B.FORCE_KV_FLAGS = None
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
