"""The additive family (KIND_ADD, csrc/kv_directadd.hpp) beside the two ways the same work ran before, in one process on one GPU, through the kernel API
(``op @ V`` without autograd: point preparation + product, as a solver iteration pays for it):
  (a) ``AdditiveStructureKernel(base, num_dims=d)``: ONE fused operator -- d one-dimensional covariances per pair, one contraction;
  (b) the same covariance as ``AdditiveKernel`` of d one-dimensional members (a ``SumFusedLinearOperator``): d complete fused products -- the only
      way to write the model before, and a code path this family leaves untouched;
  (c) the single-family ARD kernel of the same d (one d-dimensional covariance per pair), the kernel (a) is derived from.
n = 100 000, d in {2, 4, 8}, t in {1, 11, 65} columns, RBF and Matern-5/2.  HIP-event medians of 20 launches after a warm-up, the three alternating.
    python scripts/additive_kv_timing.py [n] [out.json]       -> profiles/additive_kv_timing.json"""
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/additive_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")


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


def base_kernel(kind, **kw):
    return g.kernels.RBFKernel(**kw) if kind == "rbf" else g.kernels.MaternKernel(nu=2.5, **kw)


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "kv": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    for kind in ("rbf", "matern52"):
        for d in (2, 4, 8):
            X = torch.rand(n, d, generator=gen).to(dev)
            ls = 0.2 + 0.15 * torch.rand(1, d, generator=gen)
            fused = g.kernels.AdditiveStructureKernel(base_kernel(kind, ard_num_dims=d), num_dims=d).to(dev)
            fused.base_kernel.lengthscale = ls
            members = []
            for q in range(d):
                mk = base_kernel(kind, active_dims=[q])
                mk.lengthscale = float(ls[0, q])
                members.append(mk)
            summed = g.kernels.AdditiveKernel(*members).to(dev)
            single = base_kernel(kind, ard_num_dims=d).to(dev)
            single.lengthscale = ls
            ops = [fused(X), summed(X), single(X)]
            assert ops[0].spec.kind == "add" and type(ops[1]).__name__ == "SumFusedLinearOperator" and ops[2].spec.kind == kind
            for t in (1, 11, 65):
                V = torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev)
                a, b = ops[0] @ V, ops[1] @ V
                agree = float(((a - b).abs().max(0).values / b.abs().max(0).values).max())
                a_ms, b_ms, c_ms = timed([lambda: ops[0] @ V, lambda: ops[1] @ V, lambda: ops[2] @ V])
                rec = {"base": kind, "d": d, "t": t, "fused_additive_ms": a_ms, "sum_of_d_members_ms": b_ms, "single_family_ard_ms": c_ms,
                       "sum_over_fused": b_ms / a_ms, "fused_over_single": a_ms / c_ms, "max_rel_diff_fused_vs_sum": agree}
                print(json.dumps(rec), flush=True)
                out["kv"].append(rec)
            del X, ops, V
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
