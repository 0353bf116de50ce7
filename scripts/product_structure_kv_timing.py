"""The product-structure family (KIND_PS = tensor-product Matern, csrc/kv_directps.hpp) beside its two neighbours at the same n, d and t, in one
process on one GPU, through the kernel API (``op @ V`` without autograd: point preparation + product, as a solver iteration pays for it):
  (a) ``ProductStructureKernel(Matern, num_dims=d)``: ONE exponential per pair, d polynomials multiplied in registers, one contraction;
  (b) ``AdditiveStructureKernel`` over the same base (KIND_ADD): the same body and tile, d exponentials per pair;
  (c) the isotropic-distance ``MaternKernel(ard_num_dims=d)`` on the direct-difference split path (one d-dimensional distance, one square root and
      one exponential per pair; forced there with ``backend.FORCE_KV_FLAGS`` so that all three run direct differences + split contraction).
n = 100 000, d in {2, 4, 6, 8}, t in {1, 11, 33, 65} columns, Matern 1/2, 3/2, 5/2.  HIP-event medians of 20 launches after a warm-up, the three
alternating.  Then the peak device memory of ONE training step (marginal log likelihood by mBCG + SLQ, forward and backward) at n = 20 000, d = 6,
and at n = 8 000, native against the same model formed densely (``kernels.ps_dense``; where that does not fit, the failure is recorded).
    python scripts/product_structure_kv_timing.py [n] [out.json]       -> profiles/product_structure_kv_timing.json"""
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
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/product_structure_kv_timing.json"
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
warnings.simplefilter("ignore")
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


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


def single_direct(op, V):
    """The single-family product on the direct-difference split kernels (csrc/kv_directh.hpp), whatever the Gram policy would choose."""
    B.FORCE_KV_FLAGS = B.KV_SPLIT | B.KV_SPLIT_FEW
    try:
        return op @ V
    finally:
        B.FORCE_KV_FLAGS = None


out = {"n": n, "device": torch.cuda.get_device_name(0), "reps": 20, "kv": []}
gen = torch.Generator().manual_seed(0)
with torch.no_grad():
    for kind in ("matern12", "matern32", "matern52"):
        for d in (2, 4, 6, 8):
            X = torch.rand(n, d, generator=gen).to(dev)
            ls = 0.5 + 0.4 * torch.rand(1, d, generator=gen)
            kerns = [g.kernels.ProductStructureKernel(g.kernels.MaternKernel(nu=NU[kind], ard_num_dims=d), num_dims=d),
                     g.kernels.AdditiveStructureKernel(g.kernels.MaternKernel(nu=NU[kind], ard_num_dims=d), num_dims=d)]
            for k in kerns:
                k.base_kernel.lengthscale = ls
            single = g.kernels.MaternKernel(nu=NU[kind], ard_num_dims=d)
            single.lengthscale = ls
            ops = [k.to(dev)(X) for k in kerns] + [single.to(dev)(X)]
            assert ops[0].spec.kind == "ps" and ops[1].spec.kind == "add" and ops[2].spec.kind == kind
            for t in (1, 11, 33, 65):
                V = torch.randn(n, t, generator=torch.Generator().manual_seed(t)).to(dev)
                a_ms, b_ms, c_ms = timed([lambda: ops[0] @ V, lambda: ops[1] @ V, lambda: single_direct(ops[2], V)])
                rec = {"base": kind, "d": d, "t": t, "product_structure_ms": a_ms, "additive_ms": b_ms, "isotropic_direct_split_ms": c_ms,
                       "ps_over_additive": a_ms / b_ms, "ps_over_isotropic": a_ms / c_ms}
                print(json.dumps(rec), flush=True)
                out["kv"].append(rec)
            del X, ops, V


def step_peak(dense, n_step=20_000, d=6):
    """Peak device memory (bytes) of one marginal-log-likelihood evaluation with its backward pass (mBCG + SLQ branch)."""
    native_rule = g.kernels.ps_native
    if dense:
        g.kernels.ps_native = lambda *a, **k: False
    try:
        gen = torch.Generator().manual_seed(1)
        X = torch.rand(n_step, d, generator=gen).to(dev)
        y = (torch.sin(3.0 * X).prod(-1) + 0.05 * torch.randn(n_step, generator=gen).to(dev))

        class M(g.models.ExactGP):
            def __init__(self, x, yy, lik):
                super().__init__(x, yy, lik)
                self.mean_module = g.means.ZeroMean()
                self.covar_module = g.kernels.ScaleKernel(g.kernels.ProductStructureKernel(g.kernels.MaternKernel(nu=2.5, ard_num_dims=d), num_dims=d))

            def forward(self, x):
                return g.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

        lik = g.likelihoods.GaussianLikelihood().to(dev)
        m = M(X, y, lik).to(dev)
        m.covar_module.base_kernel.base_kernel.lengthscale = 0.7
        m.train()
        lik.train()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        with g.settings.max_cholesky_size(0):
            loss = -g.ExactMarginalLogLikelihood(lik, m)(m(X), y)
            loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    finally:
        g.kernels.ps_native = native_rule


out["training_step_peak_bytes"] = []
for n_step in (8_000, 20_000):
    rec = {"n": n_step, "d": 6, "base": "matern52", "native": step_peak(False, n_step), "d_x_n_x_n_float32": 4 * 6 * n_step * n_step}
    torch.cuda.empty_cache()
    try:   # (the dense form may not fit: that is recorded, not hidden)
        rec["ps_dense"] = step_peak(True, n_step)
        rec["dense_over_native"] = rec["ps_dense"] / rec["native"]
    except RuntimeError as e:
        rec["ps_dense"] = "failed: " + str(e).splitlines()[0][:160]
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    out["training_step_peak_bytes"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
