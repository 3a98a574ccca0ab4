"""-m gpu: the mutual check of the FGINN matcher (mods_ctx_match_mutual, csrc/mutual.hip).  In every test `want` is the CPU oracle's
forward list (orc.match_fginn) filtered by the numpy restatement of the contract (tests/mutual_ref.py), compared field by field with
what the library returns, the u6 and laf rows included."""
import contextlib

import numpy as np
import pytest

import mutual_ref as mr
import orc
import synth

pytestmark = pytest.mark.gpu

TF = ("q", "t", "t_bad", "t_2nd", "d1", "d2", "d2nd", "ratio")
# the sweep's geometry (csrc/mutual.hip): MU_TILE queries per LDS tile, at least MU_MIN_TPS tiles per share of the query list, at most
# MU_MAX_SPLITS shares - one share up to 256 queries, tiles per share growing past 64 * 256 = 16384 queries
MU_TILE, MU_MIN_TPS, MU_MAX_SPLITS = 64, 4, 64


def _rand_regions(n, seed, w=800, h=600):
    """test_gpu_match.py's recipe"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, orc.REGION_DTYPE)
    r["x"] = rng.uniform(1, w - 1, n).astype(np.float32)
    r["y"] = rng.uniform(1, h - 1, n).astype(np.float32)
    r["s"] = 2.0; r["a11"] = 1.0; r["a22"] = 1.0
    v = rng.gamma(0.6, 40.0, (n, 128))
    r["desc"] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return r


@contextlib.contextmanager
def _mode(ctx, mode):
    """the shared context goes back to mode 0 whatever happens"""
    ctx.set_match_mutual(mode)
    try:
        yield
    finally:
        ctx.set_match_mutual(0)


def _want(q, t, mode, ratio=0.8, contrad=10.0, nn=50):
    fwd = orc.match_fginn(q, t, ratio, contrad, nn)
    return fwd, mr.mutual_filter(fwd, q, t, mode, ratio, contrad)


def _assert_same(got, u6, laf, want, q, t):
    assert len(got) == len(want), (len(got), len(want))
    for f in TF:
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(u6, mr.u6_rows(want, q, t))
    assert np.array_equal(laf, mr.laf_rows(want, q, t))


def _check(ctx, q, t, mode, ratio=0.8, contrad=10.0, nn=50, dropped=True, kept=True, stricter=False):
    """one search under `mode` against the filtered oracle; dropped / kept: the reference itself must drop / keep something;
    stricter: something must survive mode 1 and fall in mode 2.  Returns (forward, want)."""
    fwd, want = _want(q, t, mode, ratio, contrad, nn)
    if dropped:
        assert len(want) < len(fwd), "the case drops nothing"
    if kept:
        assert len(want) > 0, "the case keeps nothing"
    if stricter:
        k1, k2 = mr.keep_mask(fwd, q, t, 1, ratio, contrad), mr.keep_mask(fwd, q, t, 2, ratio, contrad)
        assert (k1 & ~k2).any(), "nothing is kept in mode 1 and dropped in mode 2"
    with _mode(ctx, mode):
        got, u6 = ctx.match_fginn(q, t, ratio, contrad, nn)
        laf = ctx.last_laf
        counts = ctx.match_mutual_counts()
    _assert_same(got, u6, laf, want, q, t)
    assert counts == (len(fwd), len(want))
    return fwd, want


def random_case(nq, nt, seed):
    """Random lists with planted matches: a third of the shorter list's length as queries that copy a train with a little noise (kept by
    the check), and pairs of queries that copy one train's descriptor exactly ("twins": d = 0 for both) - the even pairs within
    contradDist of each other, the odd ones far apart."""
    rng = np.random.default_rng(seed + 7000)
    q, t = _rand_regions(nq, seed), _rand_regions(nt, seed + 100)
    m = min(nq, nt)
    n_single = m // 3
    for i in range(n_single):
        q["desc"][i] = np.clip(t["desc"][i].astype(np.int16) + rng.integers(-2, 3, 128), 0, 255).astype(np.uint8)
    n_pairs = min((nq - n_single) // 2, nt - n_single, 16)
    for p in range(n_pairs):
        a, b, tr = n_single + 2 * p, n_single + 2 * p + 1, n_single + p
        q["desc"][a] = q["desc"][b] = t["desc"][tr]
        if p % 2 == 0:
            q["x"][b], q["y"][b] = q["x"][a] + 3.0, q["y"][a] + 4.0          # 5 apart
        else:
            q["x"][b], q["y"][b] = (q["x"][a] + 400.0) % 800.0, q["y"][a]
    return q, t


@pytest.mark.parametrize("nq,nt,seed", [(1, 1, 1), (1, 2, 2), (5, 3, 3), (33, 31, 4), (300, 257, 5), (1000, 1500, 6)])
@pytest.mark.parametrize("mode", [1, 2])
def test_mutual_random(gpu_ctx, nq, nt, seed, mode):
    q, t = random_case(nq, nt, seed)
    for ratio in (0.8, 0.95):
        _check(gpu_ctx, q, t, mode, ratio, dropped=nq >= 33, kept=nq >= 300, stricter=mode == 2 and nq >= 33)


def tiny_alphabet_case(nq, nt, rng):
    """test_match_ties_and_parity's lists: many queries at exactly the same distance from a train, the index decides"""
    q, t = _rand_regions(nq, 1000 + nq), _rand_regions(nt, 2000 + nt)
    q["desc"] = rng.integers(0, 3, (nq, 128)).astype(np.uint8) * 40
    t["desc"] = rng.integers(0, 3, (nt, 128)).astype(np.uint8) * 40
    t["desc"][::7, :3] += 1
    q["desc"][nq // 2:] = q["desc"][: nq - nq // 2]        # every query of the first half has an exact twin later in the list
    return q, t


@pytest.mark.parametrize("contrad", [10.0, 1e9])
def test_mutual_ties_by_index(gpu_ctx, contrad):
    rng = np.random.default_rng(77)
    for nq, nt in ((700, 1900), (257, 95), (64, 33)):
        q, t = tiny_alphabet_case(nq, nt, rng)
        for mode in (1, 2):
            for ratio in (0.8, 0.999):
                # (ratio 0.8 accepts next to nothing on these lists; under mode 2 with contradDist 10 every accepted query has a far
                # rival at its own distance - its twin or another tie - and nothing survives)
                _check(gpu_ctx, q, t, mode, ratio, contrad, dropped=ratio > 0.9, kept=ratio > 0.9 and (mode == 1 or contrad > 10.0))


def ratio_boundary_case():
    """ratio 0.5, ratio^2 = 0.25.  Group g has a train T, a query A at d1 from it and a rival R planted at exactly d_r = 4 d1 - 1, 4 d1 or
    4 d1 + 1, 500 px from A: fl32(d1 / d_r) <= 0.25 holds from 4 d1 on, so the first is dropped in mode 2 and the others are kept; a
    fourth group has the rival at 4 d1 - 1 but 5 px away (not far: kept).  Groups are 640 000 apart in descriptor space."""
    d1s = {100: (10,), 25: (5,), 3: (1, 1, 1)}
    squares = {399: (19, 6, 1, 1), 400: (20,), 401: (20, 1), 99: (9, 3, 3), 100: (10,), 101: (10, 1), 11: (3, 1, 1), 12: (2, 2, 2), 13: (3, 2)}
    groups = []
    for d1 in (100, 25, 3):
        for off, near in ((-1, False), (0, False), (1, False), (-1, True)):
            groups.append((d1, 4 * d1 + off, near))
    n = len(groups)
    assert n <= 14
    t = _rand_regions(n, 900); q = _rand_regions(2 * n, 901)
    t["desc"][:] = 0; q["desc"][:] = 0
    for g, (d1, dr, near) in enumerate(groups):
        base = np.zeros(128, np.int64)
        base[8 * g: 8 * g + 8] = 200
        base[112:] = 100
        t["desc"][g] = base
        a, r = base.copy(), base.copy()
        for i, v in enumerate(d1s[d1]):
            a[112 + i] += v
        for i, v in enumerate(squares[dr]):
            r[120 + i] -= v
        q["desc"][2 * g], q["desc"][2 * g + 1] = a, r
        q["x"][2 * g], q["y"][2 * g] = 20.0 + 10 * g, 30.0
        q["x"][2 * g + 1], q["y"][2 * g + 1] = (23.0 + 10 * g, 34.0) if near else (20.0 + 10 * g, 530.0)
        t["x"][g], t["y"][g] = 40.0 * g + 5, 300.0
    return q, t, groups


def test_mutual_ratio_boundary(gpu_ctx):
    q, t, groups = ratio_boundary_case()
    for g, (d1, dr, near) in enumerate(groups):
        d = mr.sqdist(t["desc"][[g]], q["desc"][[2 * g, 2 * g + 1]])[0]
        assert d.tolist() == [d1, dr]
    fwd, want2 = _check(gpu_ctx, q, t, 2, 0.5, 10.0, stricter=True)
    _check(gpu_ctx, q, t, 1, 0.5, 10.0)
    for g, (d1, dr, near) in enumerate(groups):
        assert 2 * g in fwd["q"]
        assert (2 * g in want2["q"]) == (near or dr >= 4 * d1), (g, d1, dr, near)


def geometry_case(nq, nt, seed, copies=1500):
    """up to `copies` queries, anywhere in the list, are noisy copies of random trains - several per train, one of them its nearest -
    the others random; the first and the last query copy a train exactly, so a rival sits in the sweep's first row and in the last
    row of its last, partial tile"""
    rng = np.random.default_rng(seed)
    t = _rand_regions(nt, seed + 1)
    q = _rand_regions(nq, seed + 2)
    who = rng.permutation(nq)[:copies]
    src = rng.integers(0, nt, len(who))
    q["desc"][who] = np.clip(t["desc"][src].astype(np.int16) + rng.integers(-3, 4, (len(who), 128)), 0, 255).astype(np.uint8)
    q["desc"][0] = t["desc"][1]
    q["desc"][nq - 1] = t["desc"][0]
    return q, t


@pytest.mark.parametrize("nq", [MU_TILE - 1, MU_TILE, MU_TILE + 1, MU_TILE * MU_MIN_TPS - 1, MU_TILE * MU_MIN_TPS, MU_TILE * MU_MIN_TPS + 1,
                                MU_TILE * MU_MIN_TPS * MU_MAX_SPLITS - 1, MU_TILE * MU_MIN_TPS * MU_MAX_SPLITS,
                                MU_TILE * MU_MIN_TPS * MU_MAX_SPLITS + 1])
def test_mutual_tile_and_split_sizes(pkg, gpu_ctx, nq):
    big = nq > 10000
    ctx = pkg.Context(0, 512, 512, 1) if big else gpu_ctx       # (capacity: 32768 regions per list)
    q, t = geometry_case(nq, 24 if big else 40, nq)
    for mode in (1, 2):
        _check(ctx, q, t, mode, 0.8, 10.0, stricter=mode == 2)
    if big:
        ctx.close()


def test_mutual_empty_full_and_stale(gpu_ctx):
    """a search that accepts nothing, one that accepts every query, and a small search behind a large one on the same context"""
    # every train twice, the copies far apart: each query's runner-up contradicts its nearest train at the same distance
    q = _rand_regions(300, 51)
    t = _rand_regions(200, 52)
    t["desc"][100:] = t["desc"][:100]
    t["x"][100:] = (t["x"][:100] + 400.0) % 800.0
    for mode in (1, 2):
        fwd, want = _check(gpu_ctx, q, t, mode, dropped=False, kept=False)
        assert len(fwd) == 0
    q, t = _rand_regions(2000, 53), _rand_regions(500, 54)
    for mode in (1, 2):
        fwd, want = _check(gpu_ctx, q, t, mode, 0.999, 1e9)
        assert len(fwd) == 2000 and len(want) <= 500
    qs, ts = random_case(33, 31, 4)
    for mode in (1, 2):
        _check(gpu_ctx, qs, ts, mode)


def test_mutual_mode_off_again_distance_and_slices(pkg, gpu_ctx):
    q, t = random_case(300, 257, 5)
    fresh = pkg.Context(0, 640, 480, 2)
    ref, ref_u6 = fresh.match_fginn(q, t)
    ref_laf = fresh.last_laf
    with _mode(gpu_ctx, 1):
        checked, _ = gpu_ctx.match_fginn(q, t)
    assert len(checked) < len(ref)
    got, u6 = gpu_ctx.match_fginn(q, t)            # mode 0 again
    assert got.tobytes() == ref.tobytes() and u6.tobytes() == ref_u6.tobytes() and gpu_ctx.last_laf.tobytes() == ref_laf.tobytes()
    assert gpu_ctx.match_mutual_counts() == (len(ref), len(ref))
    # the Hamming matcher is never checked
    d0 = fresh.match_distance(q, t, 600.0)
    with _mode(fresh, 2):
        d2 = fresh.match_distance(q, t, 600.0)
        assert fresh.match_mutual_counts() == (len(d0[0]), len(d0[0]))
    assert len(d0[0]) > 0 and d0[0].tobytes() == d2[0].tobytes() and d0[1].tobytes() == d2[1].tobytes()
    # a slice of the query list cannot be checked
    r1, r2 = pkg.ImgRep(fresh, 1 << 12), pkg.ImgRep(fresh, 1 << 12)
    r1.append_host(q); r2.append_host(t)
    with _mode(fresh, 1):
        for b, e in ((1, 300), (0, 299), (10, 20)):
            with pytest.raises(pkg.ModsError, match="whole query list"):
                pkg.match_reps(fresh, r1, r2, b, e)
        whole, wu6, wlaf = pkg.match_reps(fresh, r1, r2)
    _assert_same(whole, wu6, wlaf, mr.mutual_filter(orc.match_fginn(q, t), q, t, 1), q, t)
    part, _, _ = pkg.match_reps(fresh, r1, r2, 10, 200)
    exp = orc.match_fginn(q[10:200], t)
    assert np.array_equal(part["q"], exp["q"] + 10) and np.array_equal(part["t"], exp["t"])
    r1.close(); r2.close(); fresh.close()


def _pair_counts(pkg, ctx, dev, w, h, mode, par):
    """(PairResult, expected count) of one mods_match_pair_dev call under `mode`"""
    with _mode(ctx, mode):
        res, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
        ra, rb = ctx.regions_fetch(0), ctx.regions_fetch(1)
        got, u6 = ctx.match_dev(0, 1, par.fginn_ratio, par.contradDist, par.nn)
        laf = ctx.last_laf
    fwd, want = _want(ra, rb, mode, par.fginn_ratio, par.contradDist, par.nn)
    assert 0 < len(want) < len(fwd)
    _assert_same(got, u6, laf, want, ra, rb)
    return res, len(want)


@pytest.mark.parametrize("mode", [1, 2])
def test_mutual_pair(pkg, mode):
    import torch
    w, h = 640, 480
    a, b, _ = synth.pair(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    pkg.ransac_pin_seed(7)
    res, n = _pair_counts(pkg, ctx, dev, w, h, mode, pkg.PairParams.default())
    pkg.ransac_pin_seed(-1)
    assert res.n_tentatives == n and res.n_inliers > 0
    ctx.close()


def test_mutual_pipeline_groups(pkg):
    """Two pairs of different list lengths in one batch of a pipeline (one grouped set of launches): a 640 x 480 pair and a 512 x 384
    one set into a flat 640 x 480 frame (a pipeline has one image size).  Each pair's counts equal its single-pair call."""
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
    for mode in (1, 2):
        pkg.ransac_pin_seed(7)
        want = [_pair_counts(pkg, ctx, x, w, h, mode, par) for x in dev]
        assert want[0][0].n_described[0] != want[1][0].n_described[0]
        pipe = pkg.Pipeline(0, w, h, par, 1, 2, 3, mutual=mode)
        order = [0, 1, 1, 0, 1, 0]
        for i, k in enumerate(order):
            pipe.submit(dev[k].data_ptr(), i)
        with pytest.raises(pkg.ModsError, match="after the first submit"):
            pipe.set_match_mutual(0)
        for i, k in enumerate(order):
            res, tag = pipe.next()
            exp, n = want[k]
            assert tag == i and res.n_tentatives == n == exp.n_tentatives, (i, k, res.n_tentatives, n)
            for f in ("n_unique", "n_inliers", "ransac_samples"):
                assert getattr(res, f) == getattr(exp, f), (f, i)
            assert list(res.n_described) == list(exp.n_described) and res.n_inliers > 0
        pipe.close()
    pkg.ransac_pin_seed(-1)
    ctx.close()


def test_mutual_ladder(pkg):
    """two steps of the single-GPU ladder under mode 1: the step's tentatives are the banks' forward list, checked"""
    import torch
    w, h = 480, 360
    a, b, _ = synth.pair(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    ctx.set_match_mutual(1)
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
    steps = [pkg.LadderStep.make((1,), 360.0), pkg.LadderStep.make((1, 2), 360.0)]
    pkg.ransac_pin_seed(7)
    res, _ = pkg.match_ladder_dev(ctx, dev.data_ptr(), w, h, steps, rep1, rep2, min_matches=10 ** 6)
    pkg.ransac_pin_seed(-1)
    ra, rb = rep1.fetch(), rep2.fetch()
    fwd, want = _want(ra, rb, 1)
    assert res.steps_done == 2 and 0 < len(want) < len(fwd)
    assert res.n_tentatives == len(want)
    rep1.close(); rep2.close(); ctx.close()
