"""The product family (KIND_PROD, csrc/kv_directp.hpp) against the kernel it is derived from, in one process on one GPU:
  (a) K V at n = 200 000 with 11 / 33 / 65 columns: Matern-5/2(1) x RBF(2) and RBF(3) x Matern-3/2(3), each beside single-family Matern-5/2 of the
      same total dimension on kv_directh (FORCE_KV_FLAGS = KV_SPLIT: direct differences + split contraction) -- the yardstick;
  (b) the bilinear derivative (the product variant of kv_grad_kernel) against kv_grad for Matern-5/2 at the same shape, per-dimension sums, 11 columns;
  (c) one marginal-log-likelihood forward + backward of ScaleKernel(Matern-5/2(time) x RBF(space)) + noise at n = 200 000 through the model API, and
      the dense path such a product took before (``product_factors`` switched off) at n = 20 000, for scale.
HIP-event medians after a warm-up, product and yardstick alternating.   python scripts/product_kv_timing.py [n] [out.json] [n_dense]
-> profiles/product_kv_timing.json"""
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd import kernels as GK  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/product_kv_timing.json"
n_dense = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")


def timed_pair(fa, fb, warm=2, reps=7):
    """Medians (ms) of two callables measured alternately."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return statistics.median(ms[0]), statistics.median(ms[1])


def single_kv(xp, V):
    old = B.FORCE_KV_FLAGS
    B.FORCE_KV_FLAGS = B.KV_SPLIT
    try:
        return B.kv(xp, xp, V)
    finally:
        B.FORCE_KV_FLAGS = old


out = {"n": n, "device": torch.cuda.get_device_name(0), "kv": [], "grad": [], "mll": {}}
gen = torch.Generator().manual_seed(0)
CASES = [("matern52(1) x rbf(2)", B.prod_code(0, 3, 2), 3, [0.5, 0.5, 0.3]),          # canonical order: the RBF columns first
         ("rbf(3) x matern32(3)", B.prod_code(0, 2, 3), 6, [0.5] * 3 + [0.6] * 3)]
for name, code, d, ls in CASES:
    X = torch.rand(n, d, generator=gen).to(dev)
    lsd = torch.tensor(ls)
    xp = B.prep_points("prod", X, lsd, X.mean(0), code)
    xs = B.prep_points("matern52", X, lsd, X.mean(0))
    for t in (11, 33, 65):
        V = torch.randn(t, B.round_up(n, 4), generator=torch.Generator().manual_seed(t)).to(dev)
        V[:, n:] = 0
        assert B.kv_flags(xp, xp, t) == B.KV_SPLIT
        p_ms, s_ms = timed_pair(lambda: B.kv(xp, xp, V), lambda: single_kv(xs, V))
        rec = {"case": name, "d": d, "t": t, "product_ms": p_ms, "matern52_directh_ms": s_ms, "ratio": p_ms / s_ms,
               "pairs_per_s_product": n * n / (p_ms * 1e-3)}
        print(json.dumps(rec), flush=True)
        out["kv"].append(rec)
    t = 11
    L = torch.randn(t, B.round_up(n, 4), generator=torch.Generator().manual_seed(100 + d)).to(dev)
    R = torch.randn(t, B.round_up(n, 4), generator=torch.Generator().manual_seed(200 + d)).to(dev)
    p_ms, s_ms = timed_pair(lambda: B.kv_grad(xp, xp, L, R, iso=False), lambda: B.kv_grad(xs, xs, L, R, iso=False), warm=1, reps=5)
    rec = {"case": name, "d": d, "t": t, "product_grad_ms": p_ms, "matern52_kv_grad_ms": s_ms, "ratio": p_ms / s_ms}
    print(json.dumps(rec), flush=True)
    out["grad"].append(rec)
    del X, xp, xs, V, L, R


class Model(g.models.ExactGP):
    def __init__(self, x, y, lik):
        super().__init__(x, y, lik)
        self.mean_module = g.means.ZeroMean()
        self.covar_module = g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5, active_dims=[0]) * g.kernels.RBFKernel(active_dims=[1, 2]))

    def forward(self, x):
        return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def mll_step(nn, reps):
    X = torch.rand(nn, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    y = (torch.sin(6.2831853 * X[:, 0]) + torch.cos(3.14159265 * X.sum(-1)) + 0.1 * torch.randn(nn, device=dev)).contiguous()
    lik = g.likelihoods.GaussianLikelihood().to(dev)
    m = Model(X, y, lik).to(dev)
    m.covar_module.base_kernel.kernels[0].lengthscale, m.covar_module.base_kernel.kernels[1].lengthscale = 0.3, 0.5
    m.covar_module.outputscale, lik.noise = 1.3, 0.1
    mll = g.ExactMarginalLogLikelihood(lik, m)
    m.train()
    lik.train()
    secs, val = [], None
    for _ in range(1 + reps):           # the first pass is the warm-up
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = mll(m(m.train_inputs[0]), m.train_targets)
        val.backward()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    op = m.covar_module(m.train_inputs[0])
    return {"n": nn, "operator": type(op).__name__, "seconds_median": statistics.median(secs[1:]), "seconds_first": secs[0], "mll": float(val)}


out["mll"]["fused_product"] = mll_step(n, 2)
print(json.dumps(out["mll"]["fused_product"]), flush=True)
torch.cuda.empty_cache()
orig = GK.product_factors
GK.product_factors = lambda *a, **k: None        # the path this product took before: the members' dense matrices multiplied elementwise
try:
    out["mll"]["dense_before"] = mll_step(n_dense, 1)
except Exception as e:  # noqa: BLE001  (a measurement for scale: report what stopped it)
    out["mll"]["dense_before"] = {"n": n_dense, "error": f"{type(e).__name__}: {str(e)[:300]}"}
finally:
    GK.product_factors = orig
print(json.dumps(out["mll"]["dense_before"]), flush=True)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
