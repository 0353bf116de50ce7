"""The kernels with derivative observations (csrc/kv_rbfgrad.hpp, csrc/kv_rbfgradgrad.hpp: one product kernel with an observation policy per
family and derivative order, a bilinear-derivative kernel per family) in one process on one GPU, every (family, order) at the same cloud,
lengthscales and column count:
  rbfgrad      RBF, value + gradient: K V over vectors of length n (d + 1) (``backend.RbfGradPlan``);
  m52grad      Matern-5/2, value + gradient, on the Matern-5/2-prepared points of the same cloud;
  rbfgradgrad  RBF, + the d non-mixed second derivatives: vectors of length n (2 d + 1) (``order=2``).
Products at n = 20 000 and 100 000, d = 1, 3 and 4, t = 1 and 11 columns; the bilinear derivative (``backend.rbfgrad_kv_grad``: the 1 + d sums) at
n = 20 000, t = 11, d = 1 and 3.  The operators differ in size, so a ratio between them is the price of a family at a given n, not a comparison of
two implementations.  HIP-event medians after a warm-up, the sides alternating; the spread (min .. max over the repetitions) of each side is
recorded with it, and with every result the SHA-256 of its bytes: inputs come from fixed seeds and no kernel here uses atomics, so two libraries
that compute the same thing print the same digests.  GPAMD_LIBRARY selects the library (an A/B against another commit's build runs this script
once per library, in fresh processes).
    python scripts/gradobs_kv_timing.py [out.json]   -> profiles/gradobs_kv_timing.json"""
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd._lib import LIB_PATH  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else "profiles/gradobs_kv_timing.json"
SIDES = {"rbfgrad": ("rbf", 1), "m52grad": ("matern52", 1), "rbfgradgrad": ("rbf", 2)}   # name -> (prepared-point family, derivative order)
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")


def timed(fns, warm=2, reps=7):
    """(median, min, max) in ms of the callables measured alternately."""
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
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def digest(x):
    return hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()


def cloud(n, d):
    """The prepared points of every family on one cloud, and the lengthscale block."""
    X = torch.rand(n, d, generator=torch.Generator().manual_seed(n + d)).to(dev)
    ls = torch.full((1, d), 0.1 if d == 1 else 0.3)
    return {f: B.prep_points(f, X, ls, X.mean(0)) for f in ("rbf", "matern52")}, B.rbfgrad_inv_ls(ls, d, dev)


def columns(t, n, c, seed):
    V = torch.zeros(t, B.round_up(n * c, 4), device=dev)
    V[:, : n * c] = torch.randn(t, n * c, generator=torch.Generator().manual_seed(seed)).to(dev)
    return V


def record(rec, fns, work):
    for name, fn, (med, lo, hi) in zip(SIDES, fns, timed(fns)):
        rec.update({f"{name}_ms": med, f"{name}_min_max_ms": [lo, hi], f"{name}_pair_columns_per_s": work / (med * 1e-3),
                    f"{name}_sha256": digest(fn())})
    print(json.dumps(rec), flush=True)
    return rec


out = {"device": torch.cuda.get_device_name(0), "library": os.path.relpath(LIB_PATH), "kv": [], "grad": []}
for n in (20_000, 100_000):
    for d in (1, 3, 4):
        preps, inv_ls = cloud(n, d)
        for t in (1, 11):
            fns = []
            for fam, order in SIDES.values():
                V = columns(t, n, order * d + 1, t)
                plan = B.RbfGradPlan(preps[fam], preps[fam], inv_ls, t, order=order)
                fns.append(lambda p=plan, v=V: p.product(v))
            out["kv"].append(record({"n": n, "d": d, "t": t}, fns, n * n * t))
n, t = 20_000, 11
for d in (1, 3):
    preps, inv_ls = cloud(n, d)
    fns = []
    for fam, order in SIDES.values():
        L, R = columns(t, n, order * d + 1, 1), columns(t, n, order * d + 1, 2)
        fns.append(lambda x=preps[fam], il=inv_ls, l=L, r=R, o=order: B.rbfgrad_kv_grad(x, x, il, l, r, order=o))
    out["grad"].append(record({"n": n, "d": d, "t": t}, fns, n * n * t))
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
