"""The planted matcher cases (tests/match_cases.py) without a GPU: the numpy restatement of the walk (tests/match_ref.py) equals the CPU
oracle on every one of them, every expectation a builder states by construction holds under it, every boundary family yields both
outcomes, every planted distance is what the builder claims, and the list lengths reach the pass-1 geometry they are meant to reach
(mods_match_grid: host arithmetic, no device).  The GPU suite (test_gpu_match_edges.py) runs the same cases."""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref
import orc

SMALL = mc.small_cases()
TILE_CASES = [(tps, short) for tps in mc.TILE_POSITION_TPS for short in (False, True)]


def check_against_reference(case, nb=None):
    """what this file asserts of one search; returns the reference's tentatives"""
    q, t, params, ex = case
    name = ex["case"]
    want = ref.match_fginn(q, t, nb=nb, **params)
    orc_want = orc.match_fginn(q, t, params["ratio"], params["contrad"], params["nn"])
    assert len(want) == len(orc_want), (name, len(want), len(orc_want))
    for f in ref.TF:
        assert np.array_equal(want[f], orc_want[f]), (name, f)
    mc.check_expectations(want, case)
    for qi, ti, d in ex["planted"]:
        got = int(ref.sqdist(q["desc"][[qi]], t["desc"][[ti]])[0, 0])
        assert got == d, (name, ex["names"][qi], ti, got, d)
    return want


@pytest.mark.parametrize("k", range(len(SMALL)), ids=[c[3]["case"].replace(" ", "_") for c in SMALL])
def test_small_case_under_the_reference(k):
    check_against_reference(SMALL[k])


def _outcomes(name, family=False):
    """(accepted, rejected) by construction over the searches called `name` (or `name, <group>`), or of the whole family"""
    acc = rej = 0
    for q, t, params, ex in SMALL:
        if ex["case"].startswith(name) if family else (ex["case"] == name or ex["case"].startswith(name + ",")):
            acc += int(((ex["t"] != mc.REJECTED) & (ex["t"] != mc.UNKNOWN)).sum())
            rej += int((ex["t"] == mc.REJECTED).sum())
    return acc, rej


def test_every_boundary_family_has_both_outcomes():
    """(the expectations themselves are checked against the reference above: these counts are of what it confirmed)"""
    for ratio in mc.RATIOS:
        for d0 in mc.RATIO_D0 + (0,) + ((mc.rounding_d0(ratio),) if mc.rounding_d0(ratio) else ()):
            acc, rej = _outcomes("ratio_boundary ratio=%g d0=%d" % (ratio, d0))
            assert acc >= 1 and rej >= 1, (ratio, d0, acc, rej)
    for cd in (5, 10):
        acc, rej = _outcomes("contrad_boundary contradDist=%g" % cd)
        assert acc == 6 and rej == 6, (cd, acc, rej)
    for nn in mc.NN_CAP_NN:
        acc, rej = _outcomes("nn_cap nn=%d" % nn)
        assert acc == sum(nn >= c + 2 for c in mc.NN_CAP_C) and acc + rej == len(mc.NN_CAP_C), (nn, acc, rej)
    # every c has its first accepting nn = c + 2 and its last rejecting nn = c + 1 in the list
    assert all(c + 1 in mc.NN_CAP_NN and c + 2 in mc.NN_CAP_NN and c + 3 in mc.NN_CAP_NN for c in mc.NN_CAP_C)
    acc, rej = _outcomes("nn_cap n_t=", family=True)
    assert acc > 0 and rej > 0
    acc, rej = _outcomes("emit_edges", family=True)
    assert rej == sum(mc.EMIT_NQ)
    acc, rej = _outcomes("many_candidates")
    assert (acc, rej) == (3, 0)


def test_ratio_boundary_worked_example():
    """d0 = 100, ratio 0.5: D* = 400; 399 near is accepted with the third train as t_bad, 399 far is rejected, 400 and 401 are accepted
    with the runner-up as t_bad wherever it lies"""
    assert ref.dstar(100, 0.5) == 400 and ref.dstar(100, 0.8) == 157 and ref.dstar(0, 0.8) == 1 and ref.dstar(1, 0.999) == 2
    assert [mc.rounding_d0(r) for r in mc.RATIOS] == [None, None, 1048668, 1048925] and ref.dstar(1048668, 0.95) == 1161959
    (q, t, params, ex), = [c for c in SMALL if c[3]["case"] == "ratio_boundary ratio=0.5 d0=100"]
    assert [int(ref.sqdist(q["desc"][[g]], t["desc"][[3 * g + 1]])[0, 0]) for g in range(6)] == [399, 399, 400, 400, 401, 401]
    assert ex["t"].tolist() == [0, mc.REJECTED, 6, 9, 12, 15] and ex["t_bad"].tolist() == [2, mc.UNKNOWN, 7, 10, 13, 16]


def test_extreme_distances():
    """the figures of the extreme descriptors: 128 * 255^2 between all 0 and all 255, and the mixes"""
    rows, kind = mc._extreme_rows()
    d = ref.sqdist(rows[:6], rows[:6])
    assert d[0, 1] == 128 * 255 * 255 == 8323200 and d[0, 2] == 4161600 and d[0, 4] == 2064512 and d[2, 4] == 2080832 and d[4, 5] == 128
    assert len({r.tobytes() for r in rows}) == len(rows) == 33
    norms = (rows.astype(np.int64) ** 2).sum(1)
    assert (norms % 2 == 1).any() and (norms % 2 == 0).any()


def _grid(pkg, n_q, n_t):
    return pkg.match_grid(n_q, n_t)


def test_match_grid_needs_no_device_and_refuses_empty_lists(pkg):
    lib = pkg.lib()
    out = (C.c_int * 3)()
    assert lib.mods_match_grid(70, 8192, out) == 0 and list(out) == [1, 256, 1]
    assert lib.mods_match_grid(1025, 32, out) == 0 and list(out) == [2, 1, 1]
    for n_q, n_t in ((0, 5), (5, 0), (-1, 5)):
        assert lib.mods_match_grid(n_q, n_t, out) == -2 and b"match_grid" in lib.mods_last_error()
    assert lib.mods_match_grid(5, 5, None) == -2


@pytest.mark.parametrize("tps,short", TILE_CASES)
def test_tile_positions_reach_the_intended_grid(pkg, tps, short):
    n_t, n_tiles, splits = mc.tile_positions_size(tps, short)
    assert (n_t + 31) // 32 == n_tiles and n_t % 32 == 21
    assert _grid(pkg, 70, n_t) == (1, splits, tps)
    assert (n_tiles % tps != 0) == (short and tps > 1)
    assert (splits % 8 == 0) == (not short or tps % 2 == 0 and tps > 1)


def test_tile_position_sizes_cover_both_split_maps():
    """both workgroup-to-split maps (split counts that are a multiple of 8 and not) occur with a short last split"""
    s = {(mc.tile_positions_size(tps, True)[2] % 8 == 0) for tps in mc.TILE_POSITION_TPS if tps > 1}
    assert s == {True, False}
    assert set(range(1, 9)) | set(range(11, 16)) == set(mc.TILE_POSITION_TPS)


def test_many_candidates_grid(pkg):
    (q, t, params, ex), = mc.many_candidates()
    assert _grid(pkg, len(q), len(t)) == (1, ex["grid"]["splits"], 1) and ex["grid"]["splits"] > mc.FIX_MAXC + 2


@pytest.mark.parametrize("tps,short", TILE_CASES)
def test_tile_positions_under_the_reference(tps, short):
    case = mc.tile_positions(tps, short)
    q, t, params, ex = case
    dist, index = ref.neighbours(q, t, params["nn"])
    want = check_against_reference(case, (dist, index))
    # all seven placements and all three kinds occur, with both outcomes
    assert len(want) == int((ex["t"] != mc.REJECTED).sum()) and 0 < len(want) < 70
    # the planted trains are the two nearest of their query, in the planted tiles
    for i in range(70):
        mine = [(ti, d) for qi, ti, d in ex["planted"] if qi == i]
        assert (int(index[i, 0]), int(dist[i, 0])) == mine[0], ex["names"][i]
        assert (int(index[i, 1]), int(dist[i, 1])) == mine[1], ex["names"][i]
    k = tps
    a, b = index[:, 0] // 32, index[:, 1] // 32           # tiles of the two nearest
    half = lambda idx: ((idx % 32) >> 2) & 1
    p = np.arange(70) % 7
    assert np.all(a[p == 0] == b[p == 0]) and np.all(half(index[p == 0, 0]) == half(index[p == 0, 1]))
    assert np.all(a[p == 1] == b[p == 1]) and np.all(half(index[p == 1, 0]) != half(index[p == 1, 1]))
    assert np.all(a[p == 2] % k == 0) and np.all(b[p == 2] % k == k - 1) and np.all(a[p == 2] // k == b[p == 2] // k)
    assert np.all(index[p == 3, 0] % 32 == 0) and np.all(index[p == 3, 1] % 32 == 31)
    assert len(t) - 1 in index[p == 4]
    splits = ex["grid"]["splits"]
    assert np.all(np.sort(np.c_[a[p == 5] // k, b[p == 5] // k], axis=1) == [0, splits - 1])
    assert np.all(dist[p == 6, 0] == dist[p == 6, 1]) and np.all(a[p == 6] // k != b[p == 6] // k) and np.all(index[p == 6, 0] < index[p == 6, 1])
