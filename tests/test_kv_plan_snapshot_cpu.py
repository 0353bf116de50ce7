"""The library's host decisions for the fused K*V launch, replayed against a recorded snapshot (tests/golden/kv_plan_snapshot.json, made by
tests/golden/make_kv_plan_snapshot.py): split count, chunk and workspace of ``gpamd_kv_plan`` for every family over a grid of dimensions, column
counts, flags and shapes, and the return codes and ``gpamd_last_error()`` texts of the single-kernel families' refusals.  The snapshot was taken
before those families moved into one table (csrc/api.hip ``one_kernel``): the table must decide what the scattered branches decided.

Without a device the plan uses the library's static occupancy table and 256 compute units; with one it asks the runtime, so the test skips itself
there (it is not a ``gpu`` test: it launches nothing)."""
import itertools
import json
import os

import pytest
import torch

from tests.golden import make_kv_plan_snapshot as G

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="with a device the plan asks the runtime for occupancies: the snapshot is of the static table")


@pytest.fixture(scope="module")
def pair():
    from gpytorch_amd._lib import lib

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kv_plan_snapshot.json")) as f:
        want = json.load(f)
    return want, json.loads(json.dumps(G.snapshot(lib())))


def test_grid_is_the_recorded_one(pair):
    want, got = pair
    assert got["grid"] == want["grid"]
    assert [len(want["plans"][str(k)]) for k in G.KINDS] == [len(G.dims_of(k)) * len(G.COLS) * len(G.FLAGS) * len(G.SHAPES) for k in G.KINDS]


@pytest.mark.parametrize("kind", G.KINDS)
def test_kv_plan_matches_snapshot(pair, kind):
    want, got = pair

    def text(snap, row):
        return row if row[0] == 0 else [row[0], snap["errors"][row[1]]]

    grid = list(itertools.product(G.dims_of(kind), G.COLS, G.FLAGS, G.SHAPES))
    diff = [(g, text(want, w), text(got, r)) for g, w, r in zip(grid, want["plans"][str(kind)], got["plans"][str(kind)]) if text(want, w) != text(got, r)]
    assert not diff, f"kind {kind}: {len(diff)} of {len(grid)} plans differ; (d, t, flags, (n, m)), recorded, now: {diff[:5]}"


def test_single_kernel_families_plan_and_refuse(pair):
    """What the snapshot must contain to be worth replaying: accepted plans of each single-kernel family, and each kind of refusal."""
    want, _ = pair
    for kind in (G.PROD, G.SM, G.ADD):
        rows = want["plans"][str(kind)]
        assert any(r[0] == 0 for r in rows) and any(r[0] != 0 for r in rows)
    joined = " | ".join(want["errors"])
    for needle in ("the product family runs on the split-contraction kernel only", "the spectral-mixture family runs on the split-contraction kernel only",
                   "the additive family runs on the split-contraction kernel only", "kv_plan: the additive family takes d in 2..8",
                   "kv_plan: the product family takes d = D_A + D_B in 2..6", "kv_plan: the spectral-mixture family takes d = the prepared width",
                   "kv: the product family is not culled", "kv: the additive family is not culled", "kv: unknown kind", "kv_ng:", "kv_sm:"):
        assert needle in joined, needle


def test_refusals_match_snapshot(pair):
    want, got = pair
    assert len(got["refusals"]) == len(want["refusals"])
    for w, r in zip(want["refusals"], got["refusals"]):
        assert (r[0], r[1], r[2], got["errors"][r[3]]) == (w[0], w[1], w[2], want["errors"][w[3]])
