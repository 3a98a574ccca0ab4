"""-m gpu: the exact k-nearest-neighbour search (csrc/knn.hip; mods_match_knn, mods_match_knn_dev, mods_match_knn_reps) against the
numpy statement of its contract, tests/match_ref.py::neighbours (pinned against a double loop in test_cpu_knn.py).  Every comparison
is array_equal on both arrays: distances and indices are defined to the bit, there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
INT_MAX = 2147483647
DMAX = 128 * 255 * 255
KS = (1, 2, 10, 50, 64)


def want_rows(q, t, k):
    """(dist, index) [n_q, k] int32 of the contract: match_ref.neighbours for K = min(k, n_t), the tail padded"""
    n_q, n_t = len(q), len(t)
    dist = np.full((n_q, k), INT_MAX, np.int32); index = np.full((n_q, k), -1, np.int32)
    K = min(k, n_t)
    if K > 0 and n_q > 0:
        d, i = ref.neighbours(q, t, K)
        dist[:, :K] = d; index[:, :K] = i
    return dist, index


def assert_rows(got, want, what=""):
    for name, g, w in (("dist", got[0], want[0]), ("index", got[1], want[1])):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            r, c = np.argwhere(g != w)[0]
            raise AssertionError("%s: %s differs first at query %d, position %d: got %d, want %d (%d entries differ)"
                                 % (what, name, r, c, g[r, c], w[r, c], int((g != w).sum())))


def clustered(n_q, n_t, rng, centres=300):
    """descriptors a few squares away from 300 centres: many small distances and near-ties"""
    cen = rng.integers(8, 248, (centres, 128))
    def members(n):
        d = cen[rng.integers(0, centres, n)].copy()
        for _ in range(3):
            d[np.arange(n), rng.integers(0, 128, n)] += rng.integers(-3, 4, n)
        return d.astype(np.uint8)
    q, t = mc.random_regions(n_q, rng), mc.random_regions(n_t, rng)
    q["desc"], t["desc"] = members(n_q), members(n_t)
    return q, t


@pytest.fixture(scope="module")
def bulk():
    """the 3000 x 2500 sets and their 64 neighbours, formed once and never modified (a shorter k is a prefix of the rows)"""
    out = {}
    for name in ("uniform", "clustered"):
        rng = np.random.default_rng(1234 if name == "uniform" else 4321)
        q, t = (mc.random_regions(3000, rng), mc.random_regions(2500, rng)) if name == "uniform" else clustered(3000, 2500, rng)
        d, i = want_rows(q, t, 64)
        d.setflags(write=False); i.setflags(write=False)
        out[name] = (q, t, d, i)
    return out


# ---- 1. small lists around every boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 127, 129])
def test_small_lists(gpu_ctx, n_q):
    """n_t around the 32-row tile and k: fewer trains than k (the padding is checked explicitly), as many, and the pad rows of the
    last tile never appear"""
    rng = np.random.default_rng(n_q)
    q = mc.random_regions(n_q, rng)
    for n_t in (1, 2, 31, 32, 33, 63, 64, 65):
        t = mc.random_regions(n_t, rng)
        for k in (1, 2, 50, 64):
            dist, index = gpu_ctx.match_knn(q, t, k)
            assert_rows((dist, index), want_rows(q, t, k), "n_q=%d n_t=%d k=%d" % (n_q, n_t, k))
            K = min(k, n_t)
            assert (index[:, K:] == -1).all() and (dist[:, K:] == INT_MAX).all()
            assert (index[:, :K] >= 0).all() and (index[:, :K] < n_t).all() and (dist[:, :K] <= DMAX).all()


def test_empty_lists(gpu_ctx):
    rng = np.random.default_rng(1)
    q, t = mc.random_regions(5, rng), mc.random_regions(7, rng)
    dist, index = gpu_ctx.match_knn(q, t[:0], 3)
    assert dist.shape == (5, 3) and (dist == INT_MAX).all() and (index == -1).all()
    dist, index = gpu_ctx.match_knn(q[:0], t, 3)
    assert dist.shape == (0, 3) and index.shape == (0, 3)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def test_ties(gpu_ctx):
    rng = np.random.default_rng(2)
    q = mc.random_regions(70, rng)
    # 200 identical trains: indices 0 .. 49, one distance
    t = mc.regions(200)
    t["desc"][:] = rng.integers(0, 256, 128, dtype=np.uint8)
    dist, index = gpu_ctx.match_knn(q, t, 50)
    assert (index == np.arange(50)[None, :]).all() and (dist == dist[:, :1]).all()
    assert_rows((dist, index), want_rows(q, t, 50), "identical trains")
    # groups of equal distance that straddle position K: 7 trains at each of d = 10, 20, ... around every query's descriptor, in a
    # shuffled order; K = 10 cuts the second group, whose lower indices win.  A query equal to several trains: d = 0 first
    qq = q[:9].copy()
    rows, planted = [], []
    for i in range(9):
        for g in range(4):
            for c in range(7):
                rows.append(mc.plant(qq["desc"][i], 10 * (g + 1), start=(11 * c + 3 * g) % 100))
                planted.append((i, 10 * (g + 1)))
        for c in range(3):
            rows.append(qq["desc"][i].copy()); planted.append((i, 0))
    order = rng.permutation(len(rows))
    t = mc.regions(len(rows))
    t["desc"] = np.array(rows, np.uint8)[order]
    owner = np.array([p[0] for p in planted])[order]; dd = np.array([p[1] for p in planted])[order]
    for k in (3, 10, 12, 64):
        dist, index = gpu_ctx.match_knn(qq, t, k)
        assert_rows((dist, index), want_rows(qq, t, k), "tie groups k=%d" % k)
        for i in range(9):
            mine = np.flatnonzero(owner == i)
            keys = sorted((int(dd[j]), int(j)) for j in mine)[:min(k, 31)]        # by construction: 3 at 0, then 7 per group
            assert [(int(d), int(j)) for d, j in zip(dist[i], index[i])][:len(keys)] == keys, (k, i)


# ---- 3. range ends ---------------------------------------------------------------------------------------------------------------
def test_range_ends(gpu_ctx):
    q = mc.regions(2)
    q["desc"][0] = 0; q["desc"][1] = 255
    t = mc.regions(40)
    t["desc"][0::2] = 255; t["desc"][1::2] = 0
    dist, index = gpu_ctx.match_knn(q, t, 64)
    assert_rows((dist, index), want_rows(q, t, 64), "range ends")
    assert (dist[0, :20] == 0).all() and (dist[0, 20:40] == DMAX).all() and (index[0, :20] == np.arange(1, 40, 2)).all()
    assert (dist[1, :20] == 0).all() and (dist[1, 20:40] == DMAX).all() and (index[1, 20:40] == np.arange(1, 40, 2)).all()
    assert (dist[:, 40:] == INT_MAX).all() and (index[:, 40:] == -1).all()


# ---- 4. order independence -------------------------------------------------------------------------------------------------------
def test_order_independence(gpu_ctx):
    """one set of 4000 trains in random order, sorted nearest first and farthest first for a probe query (farthest first makes every
    train a hit: the queue and merge path under its worst load); k = 64, one split.  Every result equals the reference on the list
    as given.  Mapped back to the original indices the three results are equal to each other and to the reference of the original
    list - except that a tie between the 64th and the 65th neighbour is decided by the index in the list as given, as the contract
    says: in such a row (found from the reference's 65 neighbours) the distances and every entry nearer than the tie are equal"""
    rng = np.random.default_rng(4)
    q, t = mc.random_regions(300, rng), mc.random_regions(4000, rng)
    d65, i65 = ref.neighbours(q, t, 65)
    want = (d65[:, :64].astype(np.int32), i65[:, :64].astype(np.int32))
    cut_tie = d65[:, 63] == d65[:, 64]
    settled = want[0] < d65[:, 63:64]              # entries no tie at the cut can touch
    settled[~cut_tie] = True
    d_probe = ref.sqdist(q["desc"][:1], t["desc"])[0]
    near = np.argsort(d_probe, kind="stable")
    gpu_ctx.knn_splits(1)
    try:
        results = []
        for name, order in (("random", np.arange(4000)), ("nearest first", near), ("farthest first", near[::-1].copy())):
            dist, index = gpu_ctx.match_knn(q, t[order], 64)
            assert_rows((dist, index), want_rows(q, t[order], 64), name + ", the list as given")
            back = order[index].astype(np.int32)
            # equal distances come out by the index in the list as given: map back, then order ties by the original index
            key = np.sort((dist.astype(np.int64) << 24) | back, axis=1)
            results.append(((key >> 24).astype(np.int32), (key & 0xFFFFFF).astype(np.int32)))
            assert np.array_equal(results[-1][0], dist), name
            assert np.array_equal(results[-1][0], want[0]), name
            assert np.array_equal(results[-1][1][settled], want[1][settled]), name
        assert all(np.array_equal(r[0], results[0][0]) and np.array_equal(r[1][settled], results[0][1][settled]) for r in results)
        # the probe's own row in the farthest-first list: its K nearest are the list's last K rows, backwards
        dist, index = gpu_ctx.match_knn(q[:1], t[near[::-1]], 64)
        assert np.array_equal(dist[0], np.sort(d_probe)[:64])
    finally:
        gpu_ctx.knn_splits(0)


# ---- 5. tile and split positions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 64])
def test_tile_and_split_positions(pkg, gpu_ctx, k):
    """the K nearest of chosen queries planted at the first and last row of a tile, at rows 31 / 32 / 33, at the first and last row of
    every split and in the list's last, partial tile - by match_cases.plant, so the expectation holds by construction - with 0 (the
    library's choice), 1, 2, 3 and 7 splits on 587 trains (19 tiles, the last of 11 rows)"""
    rng = np.random.default_rng(50 + k)
    n_t = 587
    n_tiles = (n_t + 31) // 32
    q, t = mc.random_regions(40, rng), mc.random_regions(n_t, rng)
    expect = {}
    taken = set()

    def plant_at(i, places):
        """query i: its neighbours at the given rows, distances 5, 6, ... in that order"""
        rows = []
        for n, row in enumerate(places):
            assert row not in taken and row < n_t
            taken.add(row)
            t["desc"][row] = mc.plant(q["desc"][i], 5 + n, start=(7 * n) % 100)
            rows.append((5 + n, row))
        expect[i] = rows

    # the first and the last row of every non-empty split of every forced split count, exactly; five rows per query, so that at
    # k = 5 every one of them is among its query's K nearest by construction
    edges = []
    for forced in (2, 3, 7):
        qb, splits, tps = pkg.knn_grid(len(q), n_t, k, forced)
        assert splits == forced and tps * splits >= n_tiles
        for s in range(splits):
            if s * tps < n_tiles:
                for row in (s * tps * 32, min(n_t, (s + 1) * tps * 32) - 1):
                    if row not in edges:
                        edges.append(row)
    assert {0, 319, 320, 223, 224, 447, 448, 95, 96, 479, 480, 575, 576, n_t - 1} <= set(edges)
    qi = 0
    for c in range(0, len(edges), 5):
        plant_at(qi, edges[c:c + 5])
        qi += 1
    assert all(row in taken for row in edges)
    plant_at(qi, [r for r in (0, 31, 32, 33, 63, 64) if r not in taken])               # first / last row of a tile, rows 31 / 32 / 33
    plant_at(qi + 1, [r for r in (n_t - 1, n_t - 2, 577, 576, 575) if r not in taken]) # the last, partial tile and the row before it
    qi += 2
    # k neighbours spread one per tile (and wrapped): every split holds part of the answer
    plant_at(qi, [(37 * n) % n_t for n in range(70) if (37 * n) % n_t not in taken][:64])
    want = want_rows(q, t, k)
    try:
        for forced in (0, 1, 2, 3, 7):
            gpu_ctx.knn_splits(forced)
            got = gpu_ctx.match_knn(q, t, k)
            assert_rows(got, want, "splits=%d" % forced)
            for i, rows in expect.items():
                n = min(k, len(rows))
                assert [(int(d), int(j)) for d, j in zip(got[0][i, :n], got[1][i, :n])] == rows[:n], (forced, i)
    finally:
        gpu_ctx.knn_splits(0)


# ---- 6. random bulk --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "clustered"])
@pytest.mark.parametrize("k", KS)
def test_bulk(gpu_ctx, bulk, name, k):
    q, t, d, i = bulk[name]
    assert_rows(gpu_ctx.match_knn(q, t, k), (d[:, :k], i[:, :k]), "%s k=%d" % (name, k))


def test_outputs_may_be_null_one_at_a_time(pkg, gpu_ctx, bulk):
    q, t, d, i = bulk["uniform"]
    q = q[:300]
    out = np.zeros((300, 10), np.int32)
    assert pkg.lib().mods_match_knn(gpu_ctx.h, q.ctypes.data_as(C.c_void_p), 300, t.ctypes.data_as(C.c_void_p), len(t), 10,
                                    out.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(out, i[:300, :10])
    assert pkg.lib().mods_match_knn(gpu_ctx.h, q.ctypes.data_as(C.c_void_p), 300, t.ctypes.data_as(C.c_void_p), len(t), 10,
                                    None, out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out, d[:300, :10])


# ---- 7. the reference's walk from the lists --------------------------------------------------------------------------------------
def _walk_case(gpu_ctx, q, t, params, what):
    nn = params["nn"]
    K = min(nn, len(t))
    dist, index = gpu_ctx.match_knn(q, t, K)
    want = ref.match_fginn(q, t, nb=(dist.astype(np.int64), index.astype(np.int64)), **params)
    got, _ = gpu_ctx.match_fginn(q, t, **params)
    assert len(got) == len(want), (what, len(got), len(want))
    for f in ref.TF:
        assert np.array_equal(got[f], want[f]), (what, f)
    return len(got)


def test_walk_over_the_lists_equals_the_matcher(gpu_ctx, bulk):
    """match_ref.match_fginn fed with the library's k = 50 lists equals mods_match_fginn's tentatives field by field: the matcher's
    restatement of the walk as reductions, checked against neighbour lists made on the device"""
    q, t, _, _ = bulk["clustered"]
    assert _walk_case(gpu_ctx, q[:1500], t, {"ratio": 0.8, "contrad": 10.0, "nn": 50}, "clustered") > 0
    n = 0
    for case in (mc.contrad_boundary()[0], mc.many_candidates()[0]):
        n += _walk_case(gpu_ctx, case[0], case[1], case[2], case[3]["case"])
    assert n > 0


# ---- 8. entry points agree -------------------------------------------------------------------------------------------------------
def test_entry_points_agree(pkg, gpu_ctx):
    import torch
    import orc
    from PIL import Image
    a, b = (orc.grey_of_rgb(np.asarray(Image.open(f).convert("RGB"))) for f in (G1, G6))
    h, w = a.shape
    img = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    gpu_ctx.detect_describe_dev(img.data_ptr(), 2, w, h)
    ra, rb = gpu_ctx.regions_fetch(0), gpu_ctx.regions_fetch(1)
    assert len(ra) > 900 and len(rb) > 900
    want = want_rows(ra, rb, 50)
    assert_rows(gpu_ctx.match_knn_dev(0, 1, 50), want, "match_knn_dev")
    assert_rows(gpu_ctx.match_knn(ra, rb, 50), want, "match_knn on the fetched regions")
    # an image against itself: the nearest train of a region is itself wherever its descriptor is unique
    dist, index = gpu_ctx.match_knn_dev(0, 0, 2)
    assert (dist[:, 0] == 0).all()
    unique = dist[:, 1] > 0
    assert unique.sum() > len(ra) // 2 and np.array_equal(index[unique, 0], np.flatnonzero(unique))
    assert_rows((dist, index), want_rows(ra, ra, 2), "img_q == img_t")
    rq, rt = pkg.ImgRep(gpu_ctx, 1 << 14), pkg.ImgRep(gpu_ctx, 1 << 14)
    try:
        rq.append_ctx(0); rt.append_ctx(1)
        n = len(rq)
        for q0, q1 in ((0, n), (17, 17), (17, 900)):
            got = gpu_ctx.match_knn_reps(rq, rt, 50, q0, q1)
            assert_rows(got, (want[0][q0:q1], want[1][q0:q1]), "match_knn_reps [%d, %d)" % (q0, q1))
        assert_rows(gpu_ctx.match_knn_reps(rq, rt, 50), want, "match_knn_reps, whole bank")
        for q0, q1 in ((5, 4), (-1, 3), (0, n + 1)):
            assert pkg.lib().mods_match_knn_reps(gpu_ctx.h, rq.h, q0, q1, rt.h, 5, want[0].ctypes.data_as(C.c_void_p), None) == -2
            assert pkg.lib().mods_last_error().startswith(b"match_knn_reps: bad query range")
    finally:
        rq.close(); rt.close()


def test_capacity_refusal(pkg):
    ctx = pkg.Context(0, 64, 64, 1)
    try:
        rng = np.random.default_rng(8)
        q = mc.random_regions(4, rng)
        n = 1 << 20
        out = np.zeros((4, 2), np.int32)
        # a train count above any capacity: refused before the list is read
        assert pkg.lib().mods_match_knn(ctx.h, q.ctypes.data_as(C.c_void_p), 4, q.ctypes.data_as(C.c_void_p), n * 64, 2,
                                        out.ctypes.data_as(C.c_void_p), None) == -3
        assert pkg.lib().mods_last_error().startswith(b"match_knn: list larger")
    finally:
        ctx.close()


# ---- 9. state --------------------------------------------------------------------------------------------------------------------
def test_state_is_the_search_s_own(pkg, gpu_ctx, bulk):
    q, t, d, i = bulk["clustered"]
    q1, t1 = q[:400], t[:700]
    tent, u6 = gpu_ctx.match_fginn(q1, t1, 0.9)
    laf = gpu_ctx.last_laf.copy()
    assert len(tent) > 0
    assert_rows(gpu_ctx.match_knn(q[1000:1900], t, 10), (d[1000:1900, :10], i[1000:1900, :10]), "between")
    cap = len(q1)
    tent2 = np.zeros(cap, pkg.TENT_DTYPE); u62 = np.zeros((cap, 6)); laf2 = np.zeros((cap, 14))
    n = C.c_int(-1)
    assert pkg.lib().mods_match_fetch_internal(gpu_ctx.h, tent2.ctypes.data_as(C.c_void_p), u62.ctypes.data_as(C.c_void_p),
                                               laf2.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(tent) and tent2[:n.value].tobytes() == tent.tobytes() and np.array_equal(u62[:n.value], u6)
    assert laf.shape == (len(tent), 14) and np.array_equal(laf2[:n.value], laf)
    # the mutual mode of the matcher does not concern the lists
    gpu_ctx.set_match_mutual(1)
    try:
        assert_rows(gpu_ctx.match_knn(q[:500], t, 10), (d[:500, :10], i[:500, :10]), "mutual mode 1")
    finally:
        gpu_ctx.set_match_mutual(0)
    # two contexts on one device, alternately
    other = pkg.Context(0, 640, 480, 1)
    try:
        for rnd in range(2):
            for ctx in (gpu_ctx, other):
                assert_rows(ctx.match_knn(q[:600], t, 50), (d[:600, :50], i[:600, :50]), "two contexts, round %d" % rnd)
    finally:
        other.close()


def test_stage_timers(gpu_ctx, bulk):
    q, t, d, i = bulk["uniform"]
    try:
        gpu_ctx.timing_enable(["knn", "knn_sweep", "match"]); gpu_ctx.timing_reset()
        for _ in range(2):
            gpu_ctx.match_knn(q, t, 10)
        ms, launches, _ = gpu_ctx.timing_read("knn")
        ms_sweep, launches_sweep, _ = gpu_ctx.timing_read("knn_sweep")
        assert launches == 2 and launches_sweep == 2 and 0 < ms_sweep < ms
        assert gpu_ctx.timing_read("match")[1] == 0
    finally:
        gpu_ctx.timing_enable([])


# ---- 10. next to fp64 work -------------------------------------------------------------------------------------------------------
def test_next_to_fp64_work(pkg, gpu_ctx, bulk):
    """a smoke check of the co-residency rule (the guard is test_cpu_knn.py: the sweep owns its SIMDs): LO-RANSAC on a fixed list
    with a pinned seed gives the same model and inliers before and after a search"""
    q, t, d, i = bulk["uniform"]
    rng = np.random.default_rng(5)
    H = np.array([[1.05, 0.08, 12.0], [-0.06, 0.97, -7.0], [8e-5, -4e-5, 1.0]])
    x1 = rng.uniform(0, 1000.0, (3000, 2))
    p = np.c_[x1, np.ones(3000)] @ H.T
    x2 = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (3000, 2))
    x2[rng.permutation(3000)[:1800]] = rng.uniform(0, 1000.0, (1800, 2))           # 40 % inliers
    u = np.c_[x1, np.ones(3000), x2, np.ones(3000)]
    mask1, H1, n1, _ = pkg.loransac_h(u, None, seed_time=1)
    assert_rows(gpu_ctx.match_knn(q, t, 50), (d[:, :50], i[:, :50]), "between two verifications")
    mask2, H2, n2, _ = pkg.loransac_h(u, None, seed_time=1)
    assert n1 == n2 > 1000 and np.array_equal(mask1, mask2) and np.array_equal(H1, H2)
