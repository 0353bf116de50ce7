"""Exact tile culling of the piecewise-polynomial family (settings.compact_support_culling) on the 3droad-shaped cloud of
scripts/reference_workloads.py (what `bench.py --config road3d` builds): one fused K*V with 11 and 65 columns,
  (a) Matern-5/2, every tile, lengthscale 0.05                     -- the code as it was: the yardstick
  (b) the new family at q = 2, culling off, at the same lengthscale
  (c) the new family, culling on, at the lengthscale whose support radius equals the distance at which (a) falls to 1e-7 -- the cutoff of the
      0.05-lengthscale case of DESIGN 3.1f --, with the share of (row block, tile) pairs that survive; and the same with culling off.
Medians of HIP-event times after a warm-up.   python scripts/compact_support_timing.py [n] [out.json]  -> profiles/pp_kv_timing.json"""
import json
import math
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
import gpytorch_amd as g  # noqa: E402
from gpytorch_amd import backend as B  # noqa: E402
from reference_workloads import road_like  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 217_437
path = sys.argv[2] if len(sys.argv) > 2 else "profiles/pp_kv_timing.json"
dev = torch.device("cuda:0")
X, _ = road_like(n, 0)
Xd = X.to(dev)
Q = 2


def timed(fn, warm=2, reps=9):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


warnings.simplefilter("ignore")
LS = 0.05
# Matern-5/2 at LS falls to 1e-7 at sqrt(far_sq_cutoff) prepared units = that many * LS / sqrt(5) input units: the support radius of (c)
LS_C = math.sqrt(B.far_sq_cutoff("matern52", 1e-7)) * LS / math.sqrt(5.0)
code = B.pp_code(3, Q)
clouds = {
    "a_matern52": B.prep_points("matern52", Xd, torch.tensor([LS]), Xd.mean(0)),
    "b_pp": B.prep_points("pp", Xd, torch.tensor([LS]), Xd.mean(0), code),
    "c_pp": B.prep_points("pp", Xd, torch.tensor([LS_C]), Xd.mean(0), code),
}
out = {"n": n, "q": Q, "lengthscale_a_b": LS, "lengthscale_c": LS_C, "device": torch.cuda.get_device_name(0), "runs": []}
for t in (11, 65):
    V = torch.randn(t, B.round_up(n, 4), generator=torch.Generator().manual_seed(t)).to(dev)
    V[:, n:] = 0
    rec = {"t": t}
    with g.settings.compact_support_culling(False):
        for name, xp in clouds.items():
            assert B.far_cull(xp, xp) is None
            rec[f"{name}_every_tile_ms"] = timed(lambda: B.kv(xp, xp, V))
            rec[f"{name}_gram_mode"] = B.gram_mode(xp, xp)
        ref = B.kv(clouds["c_pp"], clouds["c_pp"], V)
    for name in ("b_pp", "c_pp"):
        xp = clouds[name]
        assert B.far_cull(xp, xp) == 1.0
        rec[f"{name}_culled_ms"] = timed(lambda: B.kv(xp, xp, V))
        rec[f"{name}_kept_fraction_512"] = B.far_kept_fraction(xp, xp, 1.0, 512)
    got = B.kv(clouds["c_pp"], clouds["c_pp"], V)
    rec["c_culled_vs_every_tile_max_rel"] = float((got - ref)[:, :n].abs().max() / ref.abs().max())
    a = rec["a_matern52_every_tile_ms"]
    rec["b_over_a"] = rec["b_pp_every_tile_ms"] / a
    rec["c_over_a"] = rec["c_pp_culled_ms"] / a
    rec["expectation_b_le_1p3_a"] = rec["b_over_a"] <= 1.3
    rec["expectation_c_lt_a"] = (rec["c_over_a"] < 1.0) if rec["c_pp_kept_fraction_512"] < B.FAR_FEW_MAX_KEPT else None
    print(json.dumps(rec), flush=True)
    out["runs"].append(rec)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
