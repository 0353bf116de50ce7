"""The spectral-mixture family (KIND_SM, csrc/kv_directsm.hpp) beside what exists without it, in one process on one GPU, at n = 200 000, d = 1, Q = 4 with
11 and 65 columns:
  fused  K V of the one fused spectral-mixture operator;
  (a)    K V of single-family RBF on kv_directh (FORCE_KV_FLAGS = KV_SPLIT: direct differences + split contraction), the kernel this one's body is;
  (b)    the composition  K V = sum_q w_q (C_q K_q C_q + S_q K_q S_q) V  from Q existing RBF operators (lengthscale 1 / (2 pi sigma_q), their
         own launch policy), each with the 2 t columns [c_q o V | s_q o V], the elementwise products included -- the yardstick: fused / (b) is expected
         well below 1;
and one marginal-log-likelihood forward + backward of ExactGP(SpectralMixtureKernel(4)) through the model API (a single pass: it includes first-launch
costs).  HIP-event medians after a warm-up, the two sides of a comparison alternating.   python scripts/sm_kv_timing.py [n] [out.json]
-> profiles/sm_kv_timing.json"""
import json
import math
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402
from gpytorch_amd import backend as B  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/sm_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")
Q = 4
W, MU, SIGMA = [0.5, 0.8, 0.3, 0.6], [0.7, 1.9, 3.1, 5.2], [0.9, 1.2, 1.0, 1.4]


def timed(fns, warm=2, reps=7):
    """Medians (ms) of the callables measured alternately."""
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


def rbf_directh(xp, V):
    old = B.FORCE_KV_FLAGS
    B.FORCE_KV_FLAGS = B.KV_SPLIT
    try:
        return B.kv(xp, xp, V)
    finally:
        B.FORCE_KV_FLAGS = old


out = {"n": n, "Q": Q, "d": 1, "device": torch.cuda.get_device_name(0), "kv": [], "mll": {}}
gen = torch.Generator().manual_seed(0)
X = torch.rand(n, 1, generator=gen).to(dev)
w, mu, sigma = torch.tensor(W), torch.tensor(MU).reshape(Q, 1), torch.tensor(SIGMA).reshape(Q, 1)
theta = B.sm_theta(w, mu, sigma).to(dev)
xsm = B.prep_points("sm", X, torch.ones(1, 1), X.mean(0), theta)
scale = torch.tensor([float(w.sum())], device=dev)
xrbf = [B.prep_points("rbf", X, torch.tensor(1.0 / (2.0 * math.pi * s)), X.mean(0)) for s in SIGMA]
ld = B.round_up(n, 4)
phase = 2.0 * math.pi * ((X.double() * mu.double().to(dev).t()) % 1.0)                  # [n, Q]
cq = torch.zeros(Q, ld, device=dev)
sq = torch.zeros(Q, ld, device=dev)
cq[:, :n], sq[:, :n] = torch.cos(phase).t().float(), torch.sin(phase).t().float()
wq = w.to(dev)


def composition(V):
    t = V.shape[0]
    acc = torch.zeros_like(V)
    for q in range(Q):
        U = torch.cat([V * cq[q], V * sq[q]], 0)
        KU = B.kv(xrbf[q], xrbf[q], U)
        acc += wq[q] * (KU[:t] * cq[q] + KU[t:] * sq[q])
    return acc


for t in (11, 65):
    V = torch.randn(t, ld, generator=torch.Generator().manual_seed(t)).to(dev)
    V[:, n:] = 0
    assert B.kv_flags(xsm, xsm, t) == B.KV_SPLIT
    fused = lambda: B.kv(xsm, xsm, V, scale=scale)  # noqa: E731
    # the two forms compute the same product: compared on the way, at the size that is timed
    a, b = fused()[:, :n], composition(V)[:, :n]
    agree = float((a - b).abs().max() / b.abs().max())
    f_ms, r_ms, c_ms = timed([fused, lambda: rbf_directh(xrbf[0], V), lambda: composition(V)])
    rec = {"t": t, "fused_sm_ms": f_ms, "rbf_directh_ms": r_ms, "composition_ms": c_ms, "fused_over_rbf": f_ms / r_ms, "fused_over_composition": f_ms / c_ms,
           "pairs_per_s_fused": n * n / (f_ms * 1e-3), "fused_vs_composition_max_rel_diff": agree}
    print(json.dumps(rec), flush=True)
    out["kv"].append(rec)
del V


class Model(g.models.ExactGP):
    def __init__(self, x, y, lik):
        super().__init__(x, y, lik)
        self.mean_module = g.means.ZeroMean()
        self.covar_module = g.kernels.SpectralMixtureKernel(Q)

    def forward(self, x):
        return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


y = (torch.sin(2 * math.pi * 1.9 * X[:, 0]) + 0.5 * torch.cos(2 * math.pi * 5.2 * X[:, 0]) + 0.1 * torch.randn(n, device=dev)).contiguous()
lik = g.likelihoods.GaussianLikelihood().to(dev)
m = Model(X, y, lik).to(dev)
m.covar_module.mixture_weights, m.covar_module.mixture_means, m.covar_module.mixture_scales = w, mu.reshape(Q, 1, 1), sigma.reshape(Q, 1, 1)
lik.noise = 0.1
mll = g.ExactMarginalLogLikelihood(lik, m)
m.train()
lik.train()
torch.manual_seed(0)
torch.cuda.synchronize()
t0 = time.perf_counter()
val = mll(m(m.train_inputs[0]), m.train_targets)
val.backward()
torch.cuda.synchronize()
out["mll"] = {"n": n, "operator": type(m.covar_module(m.train_inputs[0])).__name__, "seconds_single_pass": time.perf_counter() - t0, "mll": float(val),
              "grad_finite": bool(all(torch.isfinite(p.grad).all() for p in m.parameters()))}
print(json.dumps(out["mll"]), flush=True)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
