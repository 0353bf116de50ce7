#!/usr/bin/env python3
"""Snapshot of the library's HOST decisions for the fused K*V launch: what ``gpamd_kv_plan`` answers over a grid of (kind, d, t, flags, n, m), and
the refusals of the single-kernel families (product, spectral mixture, additive, Newton-Girard additive) with their ``gpamd_last_error()`` texts
(``python tests/golden/make_kv_plan_snapshot.py`` on a machine WITHOUT a device: the plan then uses the library's static occupancy table and 256
compute units; with a device it would ask the runtime).

``kv_plan_snapshot.json`` was recorded with the library as it stood before the single-kernel families moved into one table
(csrc/api.hip ``one_kernel``); ``tests/test_kv_plan_snapshot_cpu.py`` replays ``snapshot()`` against it, so a refactor of that host code has to
reproduce every split count, chunk, workspace size, return code and message exactly.  Regenerate only when a plan is MEANT to change.

Layout: ``plans[kind]`` lists one entry per grid point in the order of ``itertools.product(dims, t, flags, nm)`` -- ``[0, S, jchunk,
workspace_floats]``, or ``[rc, index into errors]`` for a refused plan; ``refusals`` lists ``[entry point, arguments, rc, index into errors]``.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kv_plan_snapshot.json")

GRAM, SPLIT, BLOCK128, SPLIT_FEW = 1, 8, 16, 32           # include/gpamd.h GPAMD_KV_*
PROD, SM, ADD, NG = 6, 7, 8, 9                             # include/gpamd.h GPAMD_PROD ...
KINDS = list(range(9))                                     # what gpamd_kv_plan may be asked (kind 9 is planned as kind 8: recorded as a refusal)
DIMS = [1, 2, 3, 5, 8, 17]
SM_WIDTHS = [3, 9, 17, 4]                                  # d + 2 Q d for (Q, d) = (1, 1), (4, 1) or (1, 3), (8, 1); 4: no (Q, d) has that width
COLS = [1, 4, 5, 11, 33, 34, 65, 130]
FLAGS = [0, GRAM, SPLIT, GRAM | SPLIT, GRAM | SPLIT | BLOCK128, SPLIT | SPLIT_FEW]
SHAPES = [(257, 300), (2000, 2000), (500000, 500000), (9000, 36584)]


def dims_of(kind: int):
    return SM_WIDTHS if kind == SM else DIMS


def snapshot(h) -> dict:
    """Everything the fixture holds, from the loaded library ``h`` (gpytorch_amd._lib.lib())."""
    errors: list = []

    def err_index() -> int:
        msg = h.gpamd_last_error().decode()
        if msg not in errors:
            errors.append(msg)
        return errors.index(msg)

    plans = {}
    for kind in KINDS:
        rows = []
        for d, t, flags, (n, m) in itertools.product(dims_of(kind), COLS, FLAGS, SHAPES):
            S, jc, ws = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
            rc = h.gpamd_kv_plan(kind, n, m, d, t, flags, (n + 3) // 4 * 4, C.byref(S), C.byref(jc), C.byref(ws))
            rows.append([0, S.value, jc.value, ws.value] if rc == 0 else [rc, err_index()])
        plans[str(kind)] = rows

    # refusals of the single-kernel families through the launch entry points: null buffers throughout, every call is refused before any launch
    # (as tests/test_lib_abi.py::test_argument_validation_without_gpu)
    n = m = 1000
    calls = []
    for kind, kparam, d in [(PROD, 20.0, 2), (ADD, 0.0, 3)]:   # (20 = RBF x Matern-1/2, one column each)
        far = [kind, kparam, None, n, None, m, d, None, None, m, 11, None, n, 1, 1024]
        tail = [None, None, None, None, None, None]
        calls.append(("gpamd_kv_partials_far_f32", far + [GRAM | SPLIT] + tail + [23.0, None, 0]))       # a positive cutoff: not culled
        calls.append(("gpamd_kv_partials_far_f32", far + [GRAM] + tail + [0.0, None, 0]))                # no GPAMD_KV_SPLIT
        calls.append(("gpamd_kv_partials_f32", far + [0, None, None]))                                   # the same through the plain entry point
        calls.append(("gpamd_kv_partials_f32", [kind, 99.0] + far[2:] + [SPLIT, None, None]))            # a code outside the family's rule
        calls.append(("gpamd_kv_partials_f32", far[:6] + [9] + far[7:] + [SPLIT, None, None]))           # d outside the envelope
        calls.append(("gpamd_kv_f32", [kind, kparam, None, n, None, m, d, None, None, m, 11, None, None, None, 0, None, n, None, 0, GRAM, None]))
    # the spectral mixture travels with its parameter block, the Newton-Girard additive family is known to its own entry point only
    calls.append(("gpamd_kv_partials_f32", [SM, 0.0, None, n, None, m, 3, None, None, m, 11, None, n, 1, 1024, SPLIT, None, None]))
    calls.append(("gpamd_kv_partials_f32", [NG, 0.0, None, n, None, m, 3, None, None, m, 11, None, n, 1, 1024, SPLIT, None, None]))
    calls.append(("gpamd_kv_plan", [NG, n, m, 3, 11, SPLIT, n, None, None, None]))
    block = "block"                                            # (stands for a non-null host address: not dereferenced by a refused call)
    for q, d, width, blk in [(9, 1, 19, block), (5, 2, 22, block), (1, 4, 12, block), (2, 1, 5, None), (2, 1, 6, block)]:
        calls.append(("gpamd_kv_sm_partials_f32", [blk, q, d, None, n, None, m, width, None, m, 11, None, n, 1, 1024, None, None]))
    for base, d, deg, blk in [(0, 1, 1, block), (0, 9, 2, block), (0, 3, 2, None), (4, 3, 2, block), (1, 3, 0, block), (1, 3, 4, block)]:
        calls.append(("gpamd_kv_ng_partials_f32", [blk, base, d, deg, None, n, None, m, None, m, 11, None, n, 1, 1024, None, None]))
    raw = C.create_string_buffer(64)
    refusals = []
    for name, args in calls:
        rc = getattr(h, name)(*[C.addressof(raw) if a == block else a for a in args])
        assert rc != 0, f"{name}{tuple(args)} was not refused"
        refusals.append([name, args, rc, err_index()])
    return {"grid": {"kinds": KINDS, "dims": DIMS, "sm_widths": SM_WIDTHS, "t": COLS, "flags": FLAGS, "nm": [list(s) for s in SHAPES]},
            "errors": errors, "plans": plans, "refusals": refusals}


def dumps(snap: dict) -> str:
    """One line per top-level key and per kind: small, and a changed plan shows in a diff as one line."""
    lines = ["{"]
    for key in ("grid", "errors"):
        lines.append(f' "{key}": {json.dumps(snap[key])},')
    lines.append(' "plans": {')
    kinds = list(snap["plans"])
    for k in kinds:
        lines.append(f'  "{k}": {json.dumps(snap["plans"][k], separators=(",", ":"))}' + ("," if k != kinds[-1] else ""))
    lines.append(" },")
    lines.append(' "refusals": [')
    for i, r in enumerate(snap["refusals"]):
        lines.append("  " + json.dumps(r) + ("," if i + 1 < len(snap["refusals"]) else ""))
    lines.append(" ]")
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    import torch

    if torch.cuda.is_available():
        sys.exit("a device is visible: the plan would ask the runtime for occupancies; the fixture is recorded without one")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from gpytorch_amd._lib import lib

    snap = snapshot(lib())
    with open(OUT, "w") as f:
        f.write(dumps(snap))
    print(f"wrote {OUT}: {sum(len(v) for v in snap['plans'].values())} plans, {len(snap['refusals'])} refusals, {len(snap['errors'])} messages")


if __name__ == "__main__":
    main()
