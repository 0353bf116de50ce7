"""What the staging of a j-tile costs on the headline kernel: the staging arms of kv_gram_kernel (csrc/kv_gram.hpp, template parameter STG) as
csrc/tune/tune_stage.hip instantiates them side by side -- 0 = the staging up to round 6 (four dependent global round trips per tile), 1 = the
straight-line full-tile path (one), 2 = 1 + the y column's multiply-adds kept scalar.  One box, one process, n = 500 000, RBF, d = 3, 65 columns; the
arms interleaved, 6 launches each (HIP events), all arms twice; every arm's partial slabs compared BITWISE with arm 0's.
Usage: python scripts/kv_gram_stage_ab.py [out.json] [--launches N] [--rounds R] [--stamps]
  --stamps: instead of timing, run the s_memtime-stamped diagnostic builds of arms 0 and 1 (their SHARES count, not their run time) and record, per
            wave of the first 64 workgroups, the cycles between the two barriers of a tile (staging) and from the second to the next tile's first."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpytorch_amd import backend as B  # noqa: E402

argv = sys.argv[1:]


def opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = int(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


launches, rounds = opt("--launches", 6), opt("--rounds", 2)
stamps = "--stamps" in argv
if stamps:
    argv.remove("--stamps")
path = argv[0] if argv else ("kv_gram_stage_stamps.json" if stamps else "kv_gram_stage_ab.json")

dev = torch.device("cuda:0")
h = C.CDLL(os.path.join(ROOT, "gpytorch_amd", "csrc", "libgpamd_tune.so"))
f = h.gpamd_tune_stage_launch
f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
fs = h.gpamd_tune_stage_stamp_launch
fs.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
arms = [s for s in range(8) if h.gpamd_tune_stage_arms() >> s & 1]
names = {0: "0: staging up to round 6", 1: "1: straight-line full-tile staging", 2: "2: 1 + scalar y-column multiply-adds"}

n, d, t = 500_000, 3, 65
g = torch.Generator().manual_seed(0)
X = torch.rand(n, d, generator=g).to(dev)
xp = B.prep_points("rbf", X, torch.tensor(0.25), X.mean(0))
ld = B.round_up(n, 4)
V = torch.randn(t, ld, generator=g).to(dev)
S, jc, _ = B.kv_plan("rbf", n, n, d, t, B.KV_GRAM, ld)
P = torch.empty(S * t * ld, device=dev)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
out = {"n": n, "d": d, "t": t, "S": S, "jchunk": jc, "launches_per_arm_and_round": launches, "rounds": []}


def launch(stage):
    rc = f(0, stage, xp.xp.data_ptr(), n, xp.xp.data_ptr(), n, V.data_ptr(), ld, t, P.data_ptr(), ld, S, jc, st)
    assert rc == 0, rc


if stamps:
    words = h.gpamd_tune_stage_stamp_words()
    buf = (C.c_uint64 * words)()
    launch(0)
    torch.cuda.synchronize()
    ref = P.clone()
    for stage in (0, 1):
        for rep in range(2):   # the second launch counts (warm instruction cache, settled clock)
            rc = fs(stage, xp.xp.data_ptr(), n, xp.xp.data_ptr(), n, V.data_ptr(), ld, t, P.data_ptr(), ld, S, jc, st, buf)
            assert rc == 0, rc
        w = list(buf)
        stage_c = [w[4 * i] / w[4 * i + 2] for i in range(words // 4) if w[4 * i + 2]]
        contr_c = [w[4 * i + 1] / (w[4 * i + 2] - 1) for i in range(words // 4) if w[4 * i + 2] > 1]
        rec = {"arm": names[stage], "waves": len(stage_c), "tiles_per_wave": int(w[2]),
               "staging_cycles_per_tile_median": statistics.median(stage_c), "staging_cycles_per_tile_min": min(stage_c), "staging_cycles_per_tile_max": max(stage_c),
               "barrier2_to_next_barrier1_cycles_per_tile_median": statistics.median(contr_c),
               "bitwise_equal_to_arm_0": bool(torch.equal(P, ref))}
        rec["staging_share"] = rec["staging_cycles_per_tile_median"] / (rec["staging_cycles_per_tile_median"] + rec["barrier2_to_next_barrier1_cycles_per_tile_median"])
        out["rounds"].append(rec)
        print(json.dumps(rec), flush=True)
else:
    ref = None
    for rnd in range(rounds):
        rec = {}
        for stage in arms:
            launch(stage)
            torch.cuda.synchronize()
            if ref is None:
                ref = P.clone()
            same = bool(torch.equal(P, ref))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                launch(stage)
            e1.record()
            torch.cuda.synchronize()
            rec[names[stage]] = {"ms_per_launch": e0.elapsed_time(e1) / launches, "bitwise_equal_to_arm_0": same}
        out["rounds"].append(rec)
        print(json.dumps(rec), flush=True)
    if rounds >= 2:
        ms = {a: [r[a]["ms_per_launch"] for r in out["rounds"]] for a in out["rounds"][0]}
        base = statistics.mean(ms[names[0]])
        out["largest_repeat_difference_ms"] = max(max(v) - min(v) for v in ms.values())
        out["gain_over_arm_0_ms"] = {a: base - statistics.mean(v) for a, v in ms.items()}
        print(json.dumps({k: out[k] for k in ("largest_repeat_difference_ms", "gain_over_arm_0_ms")}), flush=True)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
