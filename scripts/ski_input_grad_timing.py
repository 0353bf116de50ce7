"""What input gradients cost a KISS-GP marginal log likelihood: ONE forward + backward of ``ExactMarginalLogLikelihood`` on an MI355X at n = 100 000
and 1 000 000, d = 2 (100 x 100 grid) and d = 3 (40^3 grid), default probe count, with inputs that require grad and with inputs that do not (the same
commit, the same model, alternating); and the derivative-stencil launch alone (one pair, two pairs) beside the gather at the same t.  Step times: a
host clock around work that ends in a device synchronise; launches: HIP events.
python scripts/ski_input_grad_timing.py [out.json] -> profiles/ski_input_grad_timing.json"""
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, ".")
import gpytorch_amd as g  # noqa: E402
from gpytorch_amd import backend as B  # noqa: E402
from gpytorch_amd.ski import SKIFusedLinearOperator  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/ski_input_grad_timing.json"
assert torch.cuda.is_available(), "timings are taken on the device"
dev = torch.device("cuda:0")
SHAPES = {2: [100, 100], 3: [40, 40, 40]}
LS = {2: 0.15, 3: 0.3}


class Model(g.models.ExactGP):
    """KISS-GP with an identity 'network' in front: the features are x * one, attached to the graph where ``attach`` is set."""

    def __init__(self, x, y, lik, d):
        super().__init__(x, y, lik)
        self.mean_module = g.means.ConstantMean()
        self.covar_module = g.kernels.ScaleKernel(g.kernels.GridInterpolationKernel(
            g.kernels.RBFKernel(ard_num_dims=d), grid_size=SHAPES[d], grid_bounds=[(0.0, 1.0)] * d))
        self.one = torch.nn.Parameter(torch.ones(()))
        self.attach = True

    def forward(self, x):
        z = x * self.one if self.attach else (x * self.one).detach()      # (both arms: new features, a new cloud, every step)
        return g.distributions.MultivariateNormal(self.mean_module(z), self.covar_module(z))


def events(fn, reps):
    fn()                                     # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = []
for n in (100_000, 1_000_000):
    for d in (2, 3):
        gen = torch.Generator().manual_seed(0)
        X = (0.01 + 0.98 * torch.rand(n, d, generator=gen)).to(dev)
        y = (torch.sin(5.0 * X[:, 0]) * torch.cos(3.0 * X[:, 1]) + 0.1 * torch.randn(n, generator=gen).to(dev))
        lik = g.likelihoods.GaussianLikelihood().to(dev)
        model = Model(X, y, lik, d).to(dev)
        model.covar_module.base_kernel.base_kernel.lengthscale, lik.noise = LS[d], 0.1
        model.train()
        lik.train()
        mll = g.ExactMarginalLogLikelihood(lik, model)

        def step(attach):
            model.attach = attach
            model.zero_grad(set_to_none=True)
            torch.manual_seed(0)             # the same probes for both arms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = mll(model(X), y)
            val.backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            assert not attach or bool(torch.isfinite(model.one.grad))      # (the features' gradient arrived)
            return ms, float(val)

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            step(True), step(False)          # warm-up: code objects, workspaces, the cloud
            arms = {True: [], False: []}
            for _ in range(3):               # alternating
                for attach in (True, False):
                    arms[attach].append(step(attach))
            model.attach = True
        op = model.covar_module(X * model.one)
        assert isinstance(op, SKIFusedLinearOperator) and op.a1 is not None
        cloud, _ = op.clouds()
        t = g.settings.num_trace_samples.value() + 1
        M = cloud.spec.nodes
        ga, gb = torch.randn(2, t, M, device=dev)
        ca, cb = torch.randn(2, t, B.round_up(n, 4), device=dev)
        rec = {"n": n, "d": d, "grid": SHAPES[d], "nodes": M, "t": t,
               "mll_fwd_bwd_ms_inputs_require_grad": sorted(v[0] for v in arms[True]),
               "mll_fwd_bwd_ms_inputs_detached": sorted(v[0] for v in arms[False]),
               "mll_value": arms[True][0][1],
               "gather_ms": events(lambda: B.ski_interp(cloud, ga), 20),
               "grad_one_pair_ms": events(lambda: B.ski_interp_grad(cloud, ga, ca), 20),
               "grad_two_pairs_ms": events(lambda: B.ski_interp_grad(cloud, ga, ca, gb, cb), 20)}
        rec["mll_ratio_median"] = rec["mll_fwd_bwd_ms_inputs_require_grad"][1] / rec["mll_fwd_bwd_ms_inputs_detached"][1]
        rec["grad_two_pairs_over_gather"] = rec["grad_two_pairs_ms"] / rec["gather_ms"]
        rec["grad_one_pair_over_gather"] = rec["grad_one_pair_ms"] / rec["gather_ms"]
        print(rec, flush=True)
        out.append(rec)
        del model, mll, op, cloud
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(out, open(out_path, "w"), indent=1)
