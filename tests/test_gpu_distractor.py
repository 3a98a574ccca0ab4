"""-m gpu: the distractor database of the FGINN ratio test (mods_descdb_*, mods_ctx_distractor_db; csrc/distractor.hip).  Everything
is compared to the bit with the numpy restatement of the contract (tests/distractor_ref.py on top of tests/match_ref.py)."""
import contextlib

import numpy as np
import pytest

import distractor_ref as dr
import match_cases as mc
import match_ref as ref
import synth

pytestmark = pytest.mark.gpu

TF = ref.TF
QPW, QPB = 128, 512          # csrc/distractor.hip: queries per wave and per workgroup of the sweep (DB_QPW, DB_QPB)


@contextlib.contextmanager
def _attached(ctx, full=None, half=None, splits=0):
    """the shared context goes back to no database whatever happens"""
    ctx.set_distractor_db(full, half)
    ctx.descdb_splits(splits)
    try:
        yield
    finally:
        ctx.set_distractor_db(None, None)
        ctx.descdb_splits(0)


def _assert_same(got, u6, laf, want, q, t):
    assert len(got) == len(want), (len(got), len(want))
    for f in TF:
        assert np.array_equal(got[f], want[f]), f
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(u6, ref.u6_rows(want, q, t))
    assert np.array_equal(laf, dr.laf_rows(want, q, t))


def _search(ctx, q, t, db, rows, ratio=0.8, contrad=10.0, nn=50, splits=0):
    """one host search under the database `db` (a DescDB of `rows`) against the restatement; returns (kept, forward, keep mask)"""
    want, fwd, keep, ddb = dr.match_fginn_db(q, t, rows, ratio, contrad, nn)
    with _attached(ctx, db, None, splits):
        got, u6 = ctx.match_fginn(q, t, ratio, contrad, nn)
        laf = ctx.last_laf
        counts = ctx.distractor_counts()
        got_ddb = ctx.distractor_fetch()
    _assert_same(got, u6, laf, want, q, t)
    assert counts == (len(fwd), len(want)), (counts, len(fwd), len(want))
    if len(rows):
        assert np.array_equal(got_ddb, ddb[keep])
    else:
        assert len(got_ddb) == 0
    return want, fwd, keep


# ---- mods_descdb_min_dist ---------------------------------------------------------------------------------------------------

def _db_rows(m, queries, rng):
    """m rows: random ones, duplicates, the extremes of the int8 offset and of c (all 0, all 255), and a row equal to a query"""
    rows = rng.integers(0, 256, (m, 128), dtype=np.uint8)
    if m >= 31:
        rows[5] = rows[17]; rows[m - 1] = rows[17]          # duplicate rows, one of them the last row of the last tile
        rows[3] = 0; rows[m - 2] = 255
        rows[m // 2] = queries[0]                           # d = 0
        rows[m - 3] = np.clip(queries[1].astype(np.int16) + rng.integers(-1, 2, 128), 0, 255)      # a near row in the last tile
    return rows


@pytest.mark.parametrize("m", [1, 31, 32, 33, 8191, 8192, 8193])
def test_min_dist_shapes(pkg, gpu_ctx, m):
    rng = np.random.default_rng(100 + m)
    queries = rng.integers(0, 256, (QPB + 1, 128), dtype=np.uint8)
    queries[2] = 0; queries[4] = 255
    queries[6] = queries[7]
    rows = _db_rows(m, queries, rng)
    if m == 1:
        rows[0] = queries[QPB]                              # the only row equals the last query
    db = pkg.DescDB(rows)
    assert len(db) == m
    want = dr.min_dist(queries, rows)
    assert want.min() == 0 and (m < 31 or (want[0] == 0 and want[1] <= 128))
    n_tiles = (m + 31) // 32
    # forced split counts: automatic, a short last split (3, 7), empty trailing splits (200 where the database has 256 or 257 tiles)
    for splits in (0, 3, 7, 200):
        tps = -(-n_tiles // max(1, min(splits, n_tiles))) if splits else None
        gpu_ctx.descdb_splits(splits)
        try:
            for n in (0, 1, QPW - 1, QPW, QPW + 1, QPB - 1, QPB, QPB + 1):
                got = db.min_dist(gpu_ctx, queries[QPB + 1 - n:])       # (the tail of the list: every n ends with the same query)
                assert got.dtype == np.int32 and np.array_equal(got, want[QPB + 1 - n:]), (m, splits, n, tps)
        finally:
            gpu_ctx.descdb_splits(0)
    if m == 8193:
        assert pkg.descdb_grid(m, 1, 7)[1:] == (7, 37) and 6 * 37 < 257 < 7 * 37           # the last split is short
        assert pkg.descdb_grid(m, 1, 200)[1:] == (200, 2) and 2 * 129 > 257                 # splits 129 .. 199 are empty
    db.close()


def test_min_dist_empty_database_and_large_list(pkg, gpu_ctx):
    rng = np.random.default_rng(5)
    queries = rng.integers(0, 256, (3000, 128), dtype=np.uint8)
    empty = pkg.DescDB(np.zeros((0, 128), np.uint8))
    assert len(empty) == 0 and (empty.min_dist(gpu_ctx, queries[:7]) == dr.INT_MAX).all()
    rows = rng.integers(0, 256, (5000, 128), dtype=np.uint8)
    rows[::9] = np.clip(queries[:556].astype(np.int16) + rng.integers(-2, 3, (556, 128)), 0, 255).astype(np.uint8)
    db = pkg.DescDB(rows)
    assert np.array_equal(db.min_dist(gpu_ctx, queries), dr.min_dist(queries, rows))      # six query blocks
    empty.close(); db.close()


# ---- the fp32 boundary ------------------------------------------------------------------------------------------------------

def _boundary_case(d0, d_db, rng):
    """one query of constant bytes, its train at d0 (bytes 0 .. 3 move), two far trains, and a database whose nearest row lies at
    d_db (bytes 8 .. 11 move) among random rows"""
    base = np.full(128, 20, np.uint8)
    q = mc.random_regions(1, rng); t = mc.random_regions(3, rng)
    q["desc"][0] = base
    t["desc"][0] = dr.at_distance(base, d0, 0) if d0 else base
    rows = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    rows[40] = dr.at_distance(base, d_db, 8) if d_db else base
    return q, t, rows


def test_fp32_boundary(pkg, gpu_ctx):
    rng = np.random.default_rng(9)
    assert ref.dstar(5000, 0.8) == 7813
    for d0 in (1, 3, 5000, 12345, 25600):
        ds = ref.dstar(d0, 0.8)
        assert ds <= 40000
        for d_db, kept in ((ds - 1, False), (ds, True)):
            q, t, rows = _boundary_case(d0, d_db, rng)
            assert dr.min_dist(q["desc"], rows)[0] == d_db
            db = pkg.DescDB(rows)
            want, fwd, keep = _search(gpu_ctx, q, t, db, rows)
            assert len(fwd) == 1 and fwd["d1"][0] == d0 and len(want) == int(kept), (d0, d_db)
            if kept:
                assert want["ratio"][0] == np.sqrt(ref.ratio_quotient(d0, ds)) > fwd["ratio"][0]
            db.close()
    # d0 = 0 with dDB = 0: kept, ratio unchanged; d0 > 0 with dDB = 0: dropped
    for d0, kept in ((0, True), (7, False)):
        q, t, rows = _boundary_case(d0, 0, rng)
        db = pkg.DescDB(rows)
        want, fwd, keep = _search(gpu_ctx, q, t, db, rows)
        assert len(fwd) == 1 and len(want) == int(kept)
        if kept:
            assert want["ratio"][0] == fwd["ratio"][0] == 0.0
        db.close()


# ---- a mixed list -----------------------------------------------------------------------------------------------------------

def mixed_case(seed=11, nq=300, nt=333, n_copy=200, n_rand=1000):
    """random banks of which n_copy queries have a noisy copy in the train list; the database is n_rand random rows plus a noisier
    copy of the query for every second of those, shuffled"""
    rng = np.random.default_rng(seed)
    q, t = mc.random_regions(nq, rng), mc.random_regions(nt, rng)
    who = rng.permutation(nq)[:n_copy]
    where = rng.permutation(nt)[:n_copy]
    t["desc"][where] = np.clip(q["desc"][who].astype(np.int16) + rng.integers(-3, 4, (n_copy, 128)), 0, 255).astype(np.uint8)
    extra = []
    for k, i in enumerate(who[::2]):
        amp = (2, 3, 3, 4, 5, 6)[k % 6]
        extra.append(np.clip(q["desc"][i].astype(np.int16) + rng.integers(-amp, amp + 1, 128), 0, 255).astype(np.uint8))
    rows = np.concatenate([rng.integers(0, 256, (n_rand, 128), dtype=np.uint8), np.array(extra)])
    return q, t, rows[rng.permutation(len(rows))]


def test_mixed_list(pkg, gpu_ctx):
    q, t, rows = mixed_case()
    want, fwd, keep, ddb = dr.match_fginn_db(q, t, rows)
    changed = want["ratio"] > fwd[keep]["ratio"]
    print("forward %d, dropped %d, kept %d (%d with a new ratio)" % (len(fwd), (~keep).sum(), keep.sum(), changed.sum()))
    assert len(fwd) >= 50 and (~keep).sum() * 5 >= len(fwd) and keep.sum() * 5 >= len(fwd) and changed.any() and (~changed).any()
    db = pkg.DescDB(rows)
    for splits in (0, 5):
        _search(gpu_ctx, q, t, db, rows, splits=splits)
    # the veto on a host list, in place: the forward list of a context without a database
    ftent, fu6 = gpu_ctx.match_fginn(q, t)
    flaf = gpu_ctx.last_laf
    assert ftent.tobytes() == fwd.tobytes()
    ktent, ku6, klaf, kddb = pkg.filter_distractor(gpu_ctx, db, q, ftent, fu6, flaf, 0.8)
    _assert_same(ktent, ku6, klaf, want, q, t)
    assert np.array_equal(kddb, ddb[keep])
    db.close()


# ---- no database ------------------------------------------------------------------------------------------------------------

def test_no_database(pkg, gpu_ctx):
    q, t, rows = mixed_case(seed=12)
    fwd = ref.match_fginn(q, t)
    assert len(fwd) >= 50

    def plain(ctx):
        got, u6 = ctx.match_fginn(q, t)
        _assert_same(got, u6, ctx.last_laf, fwd, q, t)
        assert ctx.distractor_counts() == (len(fwd), len(fwd)) and len(ctx.distractor_fetch()) == 0

    fresh = pkg.Context(0, 640, 480, 2)
    plain(fresh)                                            # never had a database
    empty = pkg.DescDB(np.zeros((0, 128), np.uint8))
    fresh.set_distractor_db(empty, empty)
    plain(fresh)                                            # an empty one
    db = pkg.DescDB(rows)
    fresh.set_distractor_db(db, None)
    got, _ = fresh.match_fginn(q, t)
    assert len(got) < len(fwd)
    fresh.set_distractor_db(None, None)
    plain(fresh)                                            # detached again
    # a database in the half slot alone leaves a search of whole descriptors alone, and the Hamming matcher is never vetoed
    fresh.set_distractor_db(None, db)
    plain(fresh)
    d0 = fresh.match_distance(q, t, 600.0)
    fresh.set_distractor_db(db, db)
    d1 = fresh.match_distance(q, t, 600.0)
    assert fresh.distractor_counts() == (len(d0[0]), len(d0[0])) and len(fresh.distractor_fetch()) == 0
    assert d0[0].tobytes() == d1[0].tobytes() and d0[1].tobytes() == d1[1].tobytes()
    # k-NN ignores the databases
    assert np.array_equal(fresh.match_knn(q[:40], t, 3)[0], ref.neighbours(q[:40], t, 3)[0])
    fresh.close(); empty.close(); db.close()


# ---- sharing, lifetime, refusals --------------------------------------------------------------------------------------------

def test_sharing_and_refusals(pkg, gpu_ctx):
    q, t, rows = mixed_case(seed=13)
    want, fwd, keep, ddb = dr.match_fginn_db(q, t, rows)
    db = pkg.DescDB(rows)
    a, b = pkg.Context(0, 640, 480, 2), pkg.Context(0, 640, 480, 2)
    a.set_distractor_db(db, None); b.set_distractor_db(db, db)
    for ctx in (a, b, a):
        got, u6 = ctx.match_fginn(q, t)
        _assert_same(got, u6, ctx.last_laf, want, q, t)
    # the creator's reference goes; the contexts keep the database alive
    db.close()
    got, u6 = b.match_fginn(q, t)
    _assert_same(got, u6, b.last_laf, want, q, t)
    a.close()
    got, u6 = b.match_fginn(q, t)
    _assert_same(got, u6, b.last_laf, want, q, t)
    assert np.array_equal(b.distractor_fetch(), ddb[keep])
    with pytest.raises(pkg.ModsError, match="room for 1"):
        b.distractor_fetch(cap=1)
    b.close()
    # a database made from banks: the rows of the banks in order
    r1, r2 = pkg.ImgRep(gpu_ctx, 1 << 12), pkg.ImgRep(gpu_ctx, 1 << 12)
    r1.append_host(q); r2.append_host(t)
    both = pkg.DescDB.from_reps(gpu_ctx, [r1, r2, r1])
    assert len(both) == 2 * len(q) + len(t)
    probe = rows[:300]
    assert np.array_equal(both.min_dist(gpu_ctx, probe), dr.min_dist(probe, np.concatenate([q["desc"], t["desc"]])))
    assert len(pkg.DescDB.from_reps(gpu_ctx, [])) == 0
    with pytest.raises(pkg.ModsError, match="shape"):
        pkg.DescDB(rows[:, :64])
    with pytest.raises(pkg.ModsError, match="below 1"):
        pkg.filter_distractor(gpu_ctx, both, q, fwd, ref.u6_rows(fwd, q, t), dr.laf_rows(fwd, q, t), 1.0)
    r1.close(); r2.close(); both.close()


# ---- every entry point ------------------------------------------------------------------------------------------------------

def test_reps_slices_and_mutual(pkg, gpu_ctx):
    q, t, rows = mixed_case(seed=14)
    # twins: queries that copy another query's train exactly, so that the mutual check has something to drop
    fwd0 = ref.match_fginn(q, t)
    for k in range(12):
        q["desc"][-1 - k] = t["desc"][fwd0["t"][3 * k]]
    want, fwd, keep, ddb = dr.match_fginn_db(q, t, rows)
    db = pkg.DescDB(rows)
    r1, r2 = pkg.ImgRep(gpu_ctx, 1 << 12), pkg.ImgRep(gpu_ctx, 1 << 12)
    r1.append_host(q); r2.append_host(t)
    import mutual_ref as mr
    with _attached(gpu_ctx, db):
        whole, wu6, wlaf = pkg.match_reps(gpu_ctx, r1, r2)
        _assert_same(whole, wu6, wlaf, want, q, t)
        for b, e in ((0, 300), (10, 200), (128, 129), (299, 300), (50, 50)):
            part, pu6, plaf = pkg.match_reps(gpu_ctx, r1, r2, b, e)
            sel = (want["q"] >= b) & (want["q"] < e)
            _assert_same(part, pu6, plaf, want[sel], q, t)
        # the mutual check on top gives the intersection
        for mode in (1, 2):
            mk = mr.keep_mask(fwd, q, t, mode, 0.8, 10.0)
            assert (keep & ~mk).any() and (mk & ~keep).any() and (mk & keep).any()
            both = dr.veto(fwd[mk], q, rows)[0]
            assert both.tobytes() == want[mk[keep]].tobytes()
            gpu_ctx.set_match_mutual(mode)
            try:
                got, u6 = gpu_ctx.match_fginn(q, t)
                _assert_same(got, u6, gpu_ctx.last_laf, both, q, t)
                assert gpu_ctx.distractor_counts() == (int(mk.sum()), len(both))
                assert gpu_ctx.match_mutual_counts() == (len(fwd), len(both))
            finally:
                gpu_ctx.set_match_mutual(0)
    r1.close(); r2.close(); db.close()


def dedup_case():
    """14 groups of a query and its train 640 000 apart in descriptor space, trains = queries moved by (5, 3).  Queries 0 (A) and
    1 (B) lie one pixel apart (duplicates): A's train is nearer (d0 100 against 200), so bestFGINN keeps A - until a database row
    at 200 from A lifts A's ratio to sqrt(0.5), above B's."""
    rng = np.random.default_rng(21)
    n = 14
    q, t = mc.regions(n), mc.regions(n)
    q["x"] = rng.uniform(50, 500, n).round(); q["y"] = rng.uniform(50, 400, n).round()
    q["x"][1], q["y"][1] = q["x"][0] + 1.0, q["y"][0]
    t["x"], t["y"] = q["x"] + 5.0, q["y"] + 3.0
    base = np.full((n, 128), 20, np.uint8)
    for g in range(n):
        base[g, 8 * g: 8 * g + 8] = 200
    q["desc"] = base
    for g in range(n):
        t["desc"][g] = dr.at_distance(base[g], (100, 200)[g] if g < 2 else 50 + g, 112)
    rows = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    rows[33] = dr.at_distance(base[0], 200, 116)
    return q, t, rows


def test_duplicate_filter_sees_the_new_ratios(pkg, gpu_ctx):
    q, t, rows = dedup_case()
    want, fwd, keep, ddb = dr.match_fginn_db(q, t, rows)
    assert len(fwd) == len(want) == 14 and fwd["ratio"][0] < fwd["ratio"][1] < want["ratio"][0] == np.sqrt(0.5)
    assert np.array_equal(want["ratio"][1:], fwd["ratio"][1:])
    db = pkg.DescDB(rows)
    r1, r2 = pkg.ImgRep(gpu_ctx, 1 << 8), pkg.ImgRep(gpu_ctx, 1 << 8)
    r1.append_host(q); r2.append_host(t)
    par = pkg.PairParams.default()
    assert par.dup_mode == 1 and par.dup_dist == 2.0 and par.dup_before_ransac == 1            # bestFGINN within 2 px
    pkg.ransac_pin_seed(7)
    try:
        res0, m0 = pkg.match_verify_reps(gpu_ctx, r1, r2, 0.8, par, max_matches=32)
        with _attached(gpu_ctx, db):
            res1, m1 = pkg.match_verify_reps(gpu_ctx, r1, r2, 0.8, par, max_matches=32)
    finally:
        pkg.ransac_pin_seed(-1)
    for res, m, stays, goes in ((res0, m0, 0, 1), (res1, m1, 1, 0)):
        assert res.n_tentatives == 14 and res.n_unique == 13 and res.n_inliers == 13, (res.n_tentatives, res.n_unique, res.n_inliers)
        xs = m[:, 0].tolist()
        assert q["x"][stays] in xs and q["x"][goes] not in xs, (stays, xs)
    r1.close(); r2.close(); db.close()


def _near_rows(regions, rng):
    """500 random rows and noisy copies, at four noise levels, of every third descriptor of a region list"""
    src = regions["desc"][::3]
    amp = rng.integers(1, 5, (len(src), 1))
    near = np.clip(src.astype(np.int16) + rng.integers(-4, 5, (len(src), 128)) * amp // 2, 0, 255).astype(np.uint8)
    return np.concatenate([rng.integers(0, 256, (500, 128), dtype=np.uint8), near])


def _pair_db(pkg, ctx, dev, w, h, par, seed):
    """a database that vetoes part of a synthetic pair's list: random rows and noisy copies of every third region of image 0"""
    pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
    ra = ctx.regions_fetch(0)
    return _near_rows(ra, np.random.default_rng(seed))


def _pair_want(pkg, ctx, dev, w, h, par, rows):
    """(PairResult, vetoed list) of one mods_match_pair_dev call with the database attached to ctx; mods_match_dev on the way"""
    res, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
    ra, rb = ctx.regions_fetch(0), ctx.regions_fetch(1)
    got, u6 = ctx.match_dev(0, 1, par.fginn_ratio, par.contradDist, par.nn)
    laf = ctx.last_laf
    want, fwd, keep, ddb = dr.match_fginn_db(ra, rb, rows, par.fginn_ratio, par.contradDist, par.nn)
    assert 0 < len(want) < len(fwd) and (want["ratio"] > fwd[keep]["ratio"]).any()
    _assert_same(got, u6, laf, want, ra, rb)
    assert np.array_equal(ctx.distractor_fetch(), ddb[keep])
    assert res.n_tentatives == len(want)
    return res, want


def test_pair_and_pipeline_groups(pkg):
    """mods_match_pair_dev and mods_match_dev under a database, and two pairs of different list lengths in one batch of a pipeline
    (one grouped set of launches): each pair's counts equal its single-pair call"""
    import torch
    w, h = 640, 480
    a, b, _ = synth.pair(w, h)
    c, d, _ = synth.pair(512, 384)
    cc, dd = np.full((h, w), 93.0, np.float32), np.full((h, w), 93.0, np.float32)
    cc[40:424, 60:572] = c; dd[40:424, 60:572] = d
    dev = [torch.from_numpy(np.stack(p)).cuda() for p in ((a, b), (cc, dd))]
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    ctx = pkg.Context(0, w, h, 2)
    rows = np.concatenate([_pair_db(pkg, ctx, x, w, h, par, 30 + k) for k, x in enumerate(dev)])
    db = pkg.DescDB(rows)
    ctx.set_distractor_db(db, None)
    pkg.ransac_pin_seed(7)
    try:
        want = [_pair_want(pkg, ctx, x, w, h, par, rows) for x in dev]
        assert want[0][0].n_described[0] != want[1][0].n_described[0]
        pipe = pkg.Pipeline(0, w, h, par, 1, 2, 3)
        pipe.set_distractor_db(db)
        order = [0, 1, 1, 0, 1, 0]
        for i, k in enumerate(order):
            pipe.submit(dev[k].data_ptr(), i)
        with pytest.raises(pkg.ModsError, match="after the first submit"):
            pipe.set_distractor_db(None)
        for i, k in enumerate(order):
            res, tag = pipe.next()
            exp, lst = want[k]
            assert tag == i and res.n_tentatives == len(lst) == exp.n_tentatives, (i, k, res.n_tentatives, len(lst))
            for f in ("n_unique", "n_inliers", "ransac_samples"):
                assert getattr(res, f) == getattr(exp, f), (f, i)
            assert list(res.n_described) == list(exp.n_described) and res.n_inliers > 0
        pipe.close()
    finally:
        pkg.ransac_pin_seed(-1)
    ctx.close(); db.close()


def test_ladder_slots_and_rematch(pkg):
    """one step of the single-GPU ladder with RootSIFT and HalfRootSIFT lists: the whole-descriptor slot vetoes the RootSIFT search
    alone, the half slot the HalfRootSIFT search alone; mods_match_verify_reps and mods_rematch_under_h_dev on the banks"""
    import torch
    w, h = 480, 360
    a, b, _ = synth.pair(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    steps = [pkg.LadderStep.make((1,), 360.0, half_orientation=1, fginn_half=0.8)]

    def ladder(full, half):
        rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
        ctx.set_distractor_db(full, half)
        pkg.ransac_pin_seed(7)
        res, _ = pkg.match_ladder_dev(ctx, dev.data_ptr(), w, h, steps, rep1, rep2, min_matches=10 ** 6)
        pkg.ransac_pin_seed(-1)
        counts = ctx.distractor_counts()          # of the step's last search, the HalfRootSIFT one
        return res, rep1, rep2, counts

    res0, rep1, rep2, counts0 = ladder(None, None)
    ra, rb = rep1.fetch(), rep2.fetch()
    n_root = len(ref.match_fginn(ra, rb))
    n_half = res0.n_tentatives - n_root
    assert n_root > 50 and n_half > 50 and counts0 == (n_half, n_half)
    # random rows and noisy copies of every third RootSIFT descriptor of image 1: part of its RootSIFT tentatives fall
    rng = np.random.default_rng(3)
    rows = _near_rows(ra, rng)
    want, fwd, keep, ddb = dr.match_fginn_db(ra, rb, rows)
    assert 0 < len(want) < n_root == len(fwd)
    db_root = pkg.DescDB(rows)
    res1, r1, r2, counts1 = ladder(db_root, None)
    assert r1.fetch().tobytes() == ra.tobytes() and r2.fetch().tobytes() == rb.tobytes()
    assert res1.n_tentatives == len(want) + n_half and counts1 == (n_half, n_half)
    # the banks through mods_match_verify_reps and the rematch step: the vetoed RootSIFT list
    pkg.ransac_pin_seed(7)
    resv, _ = pkg.match_verify_reps(ctx, r1, r2, 0.8)
    assert resv.n_tentatives == len(want) and resv.n_inliers > 0
    H = np.array(resv.H, np.float64).reshape(3, 3)
    x1, x2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
    x1.append_host(ra); x2.append_host(rb)
    resr, _ = pkg.rematch_under_h_dev(ctx, dev.data_ptr(), w, h, dev.data_ptr() + 4 * w * h, w, h, H, x1, x2)
    pkg.ransac_pin_seed(-1)
    qa, qb = x1.fetch(), x2.fetch()
    assert len(qa) > len(ra) and resr.n_tentatives == len(dr.match_fginn_db(qa, qb, rows)[0])
    # the half slot: rows near the HalfRootSIFT descriptors of image 1 (described once more with halfDesc) veto part of the
    # HalfRootSIFT list and leave the RootSIFT list alone
    desc = pkg.DescribeParams.default()
    desc.ori_halfMode, desc.halfDesc = 1, 1
    ctx.set_distractor_db(None, None)
    ctx.detect_describe_dev(dev.data_ptr(), 1, w, h, None, desc)
    half_rows = ctx.regions_fetch_half(0)["desc"]
    assert len(half_rows) > 100
    db_half = pkg.DescDB(half_rows[::2])
    res2, r3, r4, counts2 = ladder(None, db_half)
    assert counts2[0] == n_half and 0 <= counts2[1] < n_half, counts2
    assert res2.n_tentatives == n_root + counts2[1]
    assert len(ctx.distractor_fetch()) == counts2[1]
    ctx.set_distractor_db(None, None)
    for r in (rep1, rep2, r1, r2, r3, r4, x1, x2):
        r.close()
    db_root.close(); db_half.close(); ctx.close()


def test_ladder_group_takes_the_half_slot(pkg):
    """[Matching<i>] GroupDescriptors = HalfRootSIFT: the joined HalfRootSIFT lists of a group are a HalfRootSIFT search - the half slot
    vetoes them as it vetoes the detector's own HalfRootSIFT list (the same banks here: one detector), a whole-descriptor database
    alone leaves both as they were"""
    import torch
    w, h = 480, 360
    a, b, _ = synth.pair(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    steps = [[pkg.LadderStep.make((1,), 360.0, half_orientation=1, fginn_half=0.8)]]
    groups = [pkg.LadderGroup.make((0,), ratio=-1.0, ratio_half=0.8)]          # the RootSIFT group list is not named

    def ladder(full, half):
        rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
        ctx.set_distractor_db(full, half)
        pkg.ransac_pin_seed(7)
        res, _ = pkg.match_ladder_dets_dev(ctx, dev.data_ptr(), w, h, steps, [pkg.HessAffParams.default()], [rep1], [rep2],
                                           min_matches=10 ** 6, groups=groups, group_pos=1)
        pkg.ransac_pin_seed(-1)
        counts = ctx.distractor_counts()          # of the step's last search: the detector's own HalfRootSIFT list
        ra, rb = rep1.fetch(), rep2.fetch()
        rep1.close(); rep2.close()
        return res.n_tentatives, counts, ra, rb

    n0, counts0, ra, rb = ladder(None, None)
    n_root = len(ref.match_fginn(ra, rb))
    n_half = counts0[0]
    assert counts0 == (n_half, n_half) and n_root > 50 and n_half > 50 and n0 == n_root + 2 * n_half      # the group's list and the detector's
    rows = _near_rows(ra, np.random.default_rng(3))
    kept_root = len(dr.match_fginn_db(ra, rb, rows)[0])
    assert 0 < kept_root < n_root
    db_root = pkg.DescDB(rows)
    n1, counts1, _, _ = ladder(db_root, None)
    assert counts1 == (n_half, n_half) and n1 == kept_root + 2 * n_half
    desc = pkg.DescribeParams.default()
    desc.ori_halfMode, desc.halfDesc = 1, 1
    ctx.set_distractor_db(None, None)
    ctx.detect_describe_dev(dev.data_ptr(), 1, w, h, None, desc)
    db_half = pkg.DescDB(ctx.regions_fetch_half(0)["desc"][::2])
    n2, counts2, _, _ = ladder(None, db_half)
    assert counts2[0] == n_half and 0 <= counts2[1] < n_half, counts2
    assert n2 == n_root + 2 * counts2[1], (n2, n_root, counts2)
    n3, counts3, _, _ = ladder(db_root, db_half)
    assert counts3 == counts2 and n3 == kept_root + 2 * counts2[1]
    ctx.set_distractor_db(None, None)
    db_root.close(); db_half.close(); ctx.close()


# ---- next to fp64 work ------------------------------------------------------------------------------------------------------

def test_next_to_fp64_work(pkg, gpu_ctx):
    """a smoke check of the co-residency rule (the guard is test_cpu_distractor.py: the sweep owns its SIMDs): LO-RANSAC on a fixed
    list with a pinned seed gives the same model and inliers before and after sweeps over a database of 2^16 rows"""
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (1 << 16, 128), dtype=np.uint8)
    queries = rng.integers(0, 256, (2048, 128), dtype=np.uint8)
    db = pkg.DescDB(rows)
    want = dr.min_dist(queries, rows)
    H = np.array([[1.05, 0.08, 12.0], [-0.06, 0.97, -7.0], [8e-5, -4e-5, 1.0]])
    x1 = rng.uniform(0, 1000.0, (3000, 2))
    p = np.c_[x1, np.ones(3000)] @ H.T
    x2 = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (3000, 2))
    x2[rng.permutation(3000)[:1800]] = rng.uniform(0, 1000.0, (1800, 2))           # 40 % inliers
    u = np.c_[x1, np.ones(3000), x2, np.ones(3000)]
    mask1, H1, n1, _ = pkg.loransac_h(u, None, seed_time=1)
    for _ in range(3):
        assert np.array_equal(db.min_dist(gpu_ctx, queries), want), "between two verifications"
    mask2, H2, n2, _ = pkg.loransac_h(u, None, seed_time=1)
    assert n1 == n2 > 1000 and np.array_equal(mask1, mask2) and np.array_equal(H1, H2)
    db.close()
