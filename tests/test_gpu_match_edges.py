"""-m gpu: the forward FGINN matcher (csrc/match.hip) on the planted cases of tests/match_cases.py - its decision boundaries (the ratio
test at D* - 1 / D* / D* + 1, the contradiction test at exactly contradDist, the nn cap at K - 2 / K - 1), the ends of the integer
ranges, chosen positions of the two nearest trains in the tiles and train splits of pass 1 for every tiles-per-split count that takes
another path through the tile loop, and more candidate half tiles than the exact finish lists.  Every search equals the numpy
restatement of the walk (tests/match_ref.py, itself checked against the CPU oracle in test_cpu_match_cases.py) on all eight fields,
exactly, and the expectations the builders state by construction are asserted on the library's result directly."""
import numpy as np
import pytest

import match_cases as mc
import match_ref as ref

pytestmark = pytest.mark.gpu

SMALL = mc.small_cases()
SMALL_IDS = [c[3]["case"].replace(" ", "_") for c in SMALL]
TILE_CASES = [(tps, short) for tps in mc.TILE_POSITION_TPS for short in (False, True)]
_want = {}            # reference tentatives per small case: computed once, shared by the two runs, never modified


@pytest.fixture(scope="module")
def big_ctx(pkg):
    """room for 122 869 trains (capacity 524 288 regions per list)"""
    if pkg.lib().mods_device_count() <= 0:
        pytest.fail("no HIP device: the -m gpu tests must run on the GPU box")
    ctx = pkg.Context(0, 2048, 2048, 1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def filler():
    return mc.large_filler()


def _first_difference(got, want, f, ex):
    n = min(len(got), len(want))
    k = int(np.flatnonzero(got[f][:n] != want[f][:n])[0])
    qi = int(want["q"][k])
    return "%s: %s, field %s: got %r, want %r" % (ex["case"], ex["names"][qi] if 0 <= qi < len(ex["names"]) else qi, f, got[k], want[k])


def _check(ctx, case, want):
    q, t, params, ex = case
    got, u6 = ctx.match_fginn(q, t, **params)
    mc.check_expectations(got, case)                 # what the builder planted, on the library's own answer
    if len(got) != len(want):
        missing = sorted(set(want["q"].tolist()) ^ set(got["q"].tolist()))
        raise AssertionError("%s: %d tentatives, the reference has %d; queries that differ: %s"
                             % (ex["case"], len(got), len(want), [ex["names"][i] for i in missing[:5]]))
    for f in ref.TF:
        assert np.array_equal(got[f], want[f]), _first_difference(got, want, f, ex)
    assert np.array_equal(u6, ref.u6_rows(want, q, t)), ex["case"]


def _small_want(k):
    if k not in _want:
        q, t, params, ex = SMALL[k]
        w = ref.match_fginn(q, t, **params)
        w.setflags(write=False)
        _want[k] = w
    return _want[k]


@pytest.mark.parametrize("k", range(len(SMALL)), ids=SMALL_IDS)
def test_small_case(gpu_ctx, k):
    _check(gpu_ctx, SMALL[k], _small_want(k))


@pytest.mark.parametrize("k", range(len(SMALL)), ids=SMALL_IDS)
def test_small_case_behind_a_large_search(big_ctx, filler, k):
    """the same lists right after a 2000 x 40 000 search on the same context: the rows it left behind the end of the short lists
    (descriptors, seeds, parity words, keys) must not be seen"""
    big_ctx.match_fginn(filler[0], filler[1], 0.8)
    _check(big_ctx, SMALL[k], _small_want(k))


def test_small_cases_on_a_fresh_context(pkg):
    """... and on a context that has never run a search, in one go"""
    ctx = pkg.Context(0, 640, 480, 1)
    for k in range(len(SMALL)):
        _check(ctx, SMALL[k], _small_want(k))
    ctx.close()


@pytest.mark.parametrize("tps,short", TILE_CASES)
def test_tile_positions(pkg, big_ctx, tps, short):
    """70 queries against 8192 * tps trains or a few less: pass 1 runs `tps` tiles per split (asserted, so that a retuned grid fails
    here instead of emptying the test) - the guarded prologue steps (1 .. 4), the guarded tails of a short loop (5 .. 8), the unguarded
    four-tile body with each of its tails (11 .. 14) and a second round of it (15)"""
    case = mc.tile_positions(tps, short)
    q, t, params, ex = case
    g = ex["grid"]
    assert pkg.match_grid(len(q), len(t)) == (1, g["splits"], tps), "the pass-1 grid no longer gives %d tiles per split here" % tps
    assert (g["n_tiles"] % tps != 0) == (short and tps > 1)
    _check(big_ctx, case, ref.match_fginn(q, t, **params))
