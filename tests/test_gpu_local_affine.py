"""-m gpu: the local affine consistency filter (mods_filter_local_affine, mods_ctx_local_affine; csrc/local_affine.hip).  `want` is
always the numpy restatement of the contract (tests/local_affine_ref.py); the four diagnostic arrays and the compacted lists are
compared byte for byte - every output is an integer, a boolean or an untouched input row."""
import contextlib
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import local_affine_ref as lr
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
# csrc/local_affine.hip: rows of a sweep block, columns of an LDS tile (test_grid_constants checks them against the library)
LA_ROWS, LA_TILE = 256, 256
STRICT = dict(areaTol=0.0, rescue=0, keepSparse=0, minSupport=1)
SIZES = sorted({0, 1, 2, LA_ROWS - 1, LA_ROWS, LA_ROWS + 1, LA_TILE - 1, LA_TILE, LA_TILE + 1, 2 * LA_TILE - 1, 2 * LA_TILE,
                2 * LA_TILE + 1, 1000})


def _par(pkg, p):
    return pkg.LocalAffineParams.default(**p)


@functools.lru_cache(maxsize=None)
def random_lists(n, seed=0):
    """Clustered positions in 800 x 600 (neighbourhoods are neither empty nor everything); 60 % of the list moves under one random
    affine map per cluster, frames mapped with it, 4 % multiplicative frame noise and 0.5 px position noise, the rest lands anywhere
    with random frames; every 17th tentative repeats the positions of its predecessor (distance 0: not a neighbour), and a few
    frames are singular or not finite."""
    rng = np.random.default_rng(1000 * seed + n)
    n_cl = max(1, n // 40)
    centre = np.stack([rng.uniform(60, 740, n_cl), rng.uniform(60, 540, n_cl)], 1)
    cl = rng.integers(0, n_cl, n)
    x1 = centre[cl] + rng.normal(0, 25.0, (n, 2))
    ang = rng.uniform(0, 2 * np.pi, n)
    sc = rng.uniform(0.7, 1.4, n)
    A1 = np.stack([sc * np.cos(ang), -np.sin(ang) / sc, sc * np.sin(ang), np.cos(ang) / sc], 1)
    s1 = rng.uniform(2.0, 12.0, n)
    x2 = np.stack([rng.uniform(0, 800, n), rng.uniform(0, 600, n)], 1)
    a2 = rng.uniform(0, 2 * np.pi, n)
    A2 = np.stack([np.cos(a2), -np.sin(a2), np.sin(a2), np.cos(a2)], 1)
    s2 = rng.uniform(2.0, 12.0, n)
    M = np.eye(2) + rng.normal(0, 0.15, (n_cl, 2, 2))
    shift = rng.uniform(-60, 60, (n_cl, 2))
    t = np.flatnonzero(rng.uniform(0, 1, n) < 0.6)
    if len(t):
        x2[t] = np.einsum("nij,nj->ni", M[cl[t]], x1[t]) + shift[cl[t]] + rng.normal(0, 0.5, (len(t), 2))
        M1 = s1[t, None, None] * A1[t].reshape(-1, 2, 2)
        M2 = np.einsum("nij,njk->nik", M[cl[t]], M1) * (1.0 + rng.normal(0, 0.04, (len(t), 2, 2)))
        s2[t] = np.sqrt(np.abs(np.linalg.det(M2)))
        A2[t] = (M2 / s2[t, None, None]).reshape(-1, 4)
    tent, u6, laf = lr.make_lists(x1, x2, A1, A2, s1, s2)
    for i in range(17, n, 17):
        laf[i, 0:2] = laf[i - 1, 0:2]; laf[i, 7:9] = laf[i - 1, 7:9]
    for k, i in enumerate(range(5, n, 61)):
        if k % 4 == 0:
            laf[i, 6] = 0.0
        elif k % 4 == 1:
            laf[i, 2:6] = (1.0, 2.0, 2.0, 4.0)
        elif k % 4 == 2:
            laf[i, 13] = np.inf
        else:
            laf[i, 8] = np.nan
    u6[:, 0:2] = laf[:, 0:2]; u6[:, 3:5] = laf[:, 7:9]
    for a in (tent, u6, laf):
        a.setflags(write=False)
    return tent, u6, laf


@functools.lru_cache(maxsize=None)
def _want_random(n, strict):
    tent, u6, laf = random_lists(n)
    return lr.filter_lists(tent, u6, laf, STRICT if strict else None)


def _assert_same(got, want):
    gt, gu, gl, gd = got
    wt, wu, wl, wd = want
    for f in ("neighbours", "support", "backed", "keep"):
        assert np.array_equal(gd[f], wd[f]), (f, np.flatnonzero(gd[f] != wd[f])[:8])
    assert gd["neighbours"].dtype == np.int32 and gd["keep"].dtype == bool
    assert len(gt) == len(wt) == int(wd["keep"].sum())
    assert gt.tobytes() == wt.tobytes() and np.array_equal(gu.view(np.uint64), wu.view(np.uint64))
    assert np.array_equal(gl.view(np.uint64), np.ascontiguousarray(wl).view(np.uint64))


def test_grid_constants(pkg):
    assert pkg.local_affine_grid() == (LA_ROWS, LA_TILE)


@pytest.mark.parametrize("strict", [False, True], ids=["defaults", "strict"])
@pytest.mark.parametrize("n", SIZES)
def test_random_lists(pkg, gpu_ctx, n, strict):
    tent, u6, laf = random_lists(n)
    want = _want_random(n, strict)
    if n >= 255:       # the case judges: it keeps some, drops some, and (defaults) rescues and spares some
        k = want[3]
        assert 0 < k["keep"].sum() < n and (k["support"] > 0).any() and (k["neighbours"] > k["support"]).any()
        if not strict:
            assert (k["keep"] & (k["support"] < 3) & (k["backed"] > 0)).any() and (k["backed"] > 0).any()
    got = gpu_ctx.filter_local_affine(tent, u6, laf, _par(pkg, STRICT if strict else {}))
    _assert_same(got, want)
    assert gpu_ctx.local_affine_counts() == (n, len(want[0]))


def _hand_cases():
    five = lr.five_points()
    two = lr.two_points()
    below = np.nextafter(5.0, 0.0)
    area = lr.two_points(((50, 50), (53, 54)), (1, 2))
    deg = lr.degenerate_frames()[:3]
    res = lr.rescue_scene()
    T = lr.THRESHOLD
    yield "five", five, dict(radius=20.0)
    yield "thresholds", two, T
    yield "radius-below", two, dict(T, radius=below, minDist=below)
    yield "absTol-below", two, dict(T, absTol=below)
    yield "area-4", area, dict(T, absTol=100.0, areaTol=4.0)
    yield "area-3.9", area, dict(T, absTol=100.0, areaTol=3.9)
    yield "degenerate-area", deg, dict(radius=20.0)
    yield "degenerate-no-area", deg, dict(radius=20.0, areaTol=0.0)
    for r in (0, 1):
        for s in (0, 1):
            yield "rescue%d-sparse%d" % (r, s), res, dict(radius=20.0, areaTol=0.0, rescue=r, keepSparse=s)


@pytest.mark.parametrize("name,lists,p", list(_hand_cases()), ids=[c[0] for c in _hand_cases()])
def test_hand_cases_on_the_device(pkg, gpu_ctx, name, lists, p):
    """every hand case of test_cpu_local_affine.py (asserted there with == on the reference) through the device"""
    want = lr.filter_lists(*lists, p)
    _assert_same(gpu_ctx.filter_local_affine(*lists, _par(pkg, p)), want)
    if name == "five":
        assert want[3]["keep"].tolist() == [True, True, True, True, False]


def test_long_then_short_then_empty(pkg):
    """a long list (past the scratch a fresh context starts with: it grows), a short one and an empty one on the same context: what
    the longer list left in the scratch must not vote"""
    ctx = pkg.Context(0, 640, 480, 2)
    for n in (1500, 40, 0, 300):
        tent, u6, laf = random_lists(n, seed=3)
        _assert_same(ctx.filter_local_affine(tent, u6, laf), lr.filter_lists(tent, u6, laf))
        assert ctx.local_affine_counts()[0] == n
    ctx.close()


@contextlib.contextmanager
def _filter_on(ctx, par):
    ctx.set_local_affine(par)
    try:
        yield
    finally:
        ctx.set_local_affine(None)


PAIR_P = dict(radius=40.0, keepSparse=0)


def _verification_list(pkg, ctx, par):
    """the list the last pair of `ctx` sent to the verification with the filter off: its forward list through DuplicateFiltering"""
    tent, u6 = ctx.match_dev(0, 1, par.fginn_ratio, par.contradDist, par.nn)
    return pkg.duplicate_filter(tent, u6, par.dup_dist, par.dup_mode, ctx.last_laf)


def _same_result(a, b):
    for f in ("n_tentatives", "n_unique", "n_inliers", "ransac_samples", "ransac_lo", "ransac_rejects"):
        assert getattr(a, f) == getattr(b, f), f
    assert list(a.H) == list(b.H) and list(a.n_described) == list(b.n_described)


def _pair_expect(pkg, ctx, dev, w, h, par, seed=7):
    """(result with the filter off, result with it on, length of the reference-filtered list) of one pair; asserts the filtered call
    against the verification of the reference-filtered list"""
    pkg.ransac_pin_seed(seed)
    off, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
    tent, u6, laf = _verification_list(pkg, ctx, par)
    assert len(tent) == off.n_unique
    ft, fu, fl, d = lr.filter_lists(tent, u6, laf, PAIR_P)
    assert 0 < len(ft) < len(tent), (len(ft), len(tent))
    with _filter_on(ctx, _par(pkg, PAIR_P)):
        pkg.ransac_pin_seed(seed)
        on, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
        counts = ctx.local_affine_counts()
    assert on.n_tentatives == off.n_tentatives and on.n_unique == len(ft)
    assert counts == (len(tent), len(ft))
    p2 = type(par).from_buffer_copy(par)
    p2.dup_dist = 0.0                               # the list is past DuplicateFiltering
    vt, vu, vl, nu, H, stats = pkg.verify_tentatives(ft, fu, fl, p2, seed_time=seed)
    assert nu == len(ft) and on.n_inliers == len(vt) and on.ransac_samples == stats[0] and list(on.H) == list(H)
    return off, on, len(ft)


def test_pair_path(pkg):
    import torch
    w, h = 640, 480
    a, b, _ = synth.pair_partial(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    par = pkg.PairParams.default()
    off, on, kept = _pair_expect(pkg, ctx, dev, w, h, par)
    assert on.n_inliers > 0
    pkg.ransac_pin_seed(7)
    again, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)       # the filter is off again
    _same_result(again, off)
    # DuplicateFiltering behind RANSAC: the filter takes the search's own list
    par.dup_before_ransac = 0
    pkg.ransac_pin_seed(7)
    off0, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
    tent, u6 = ctx.match_dev(0, 1, par.fginn_ratio, par.contradDist, par.nn)
    ft = lr.filter_lists(tent, u6, ctx.last_laf, PAIR_P)[0]
    with _filter_on(ctx, _par(pkg, PAIR_P)):
        pkg.ransac_pin_seed(7)
        on0, _ = pkg.match_pair_dev(ctx, dev.data_ptr(), w, h, par)
    assert off0.n_unique == off0.n_tentatives == len(tent) and on0.n_tentatives == len(tent) and 0 < on0.n_unique == len(ft) < len(tent)
    pkg.ransac_pin_seed(-1)
    ctx.close()


@pytest.mark.parametrize("dup_first", [1, 0])
def test_pipeline_groups(pkg, dup_first):
    """Two pairs of different list lengths in one batch of a pipeline (one grouped set of launches), in a mixed submission order: each
    result equals its single-pair call with the filter on."""
    import torch
    w, h = 640, 480
    a, b, _ = synth.pair_partial(w, h)
    c, d, _ = synth.pair_partial(512, 384)
    cc, dd = np.full((h, w), 93.0, np.float32), np.full((h, w), 93.0, np.float32)
    cc[40:424, 60:572] = c; dd[40:424, 60:572] = d
    dev = [torch.from_numpy(np.stack(p)).cuda() for p in ((a, b), (cc, dd))]
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.dup_before_ransac = dup_first
    lap = _par(pkg, PAIR_P)
    ctx = pkg.Context(0, w, h, 2)
    want = []
    for x in dev:
        pkg.ransac_pin_seed(7)
        off, _ = pkg.match_pair_dev(ctx, x.data_ptr(), w, h, par)
        with _filter_on(ctx, lap):
            pkg.ransac_pin_seed(7)
            on, _ = pkg.match_pair_dev(ctx, x.data_ptr(), w, h, par)
        assert 0 < on.n_unique < off.n_unique
        want.append(on)
    assert want[0].n_described[0] != want[1].n_described[0]
    pkg.ransac_pin_seed(7)
    pipe = pkg.Pipeline(0, w, h, par, 1, 2, 3, local_affine=lap)
    order = [0, 1, 1, 0, 1, 0]
    for i, k in enumerate(order):
        pipe.submit(dev[k].data_ptr(), i)
    with pytest.raises(pkg.ModsError, match="after the first submit"):
        pipe.set_local_affine(None)
    for i, k in enumerate(order):
        res, tag = pipe.next()
        assert tag == i
        _same_result(res, want[k])
    pipe.close()
    pkg.ransac_pin_seed(-1)
    ctx.close()


def test_ladder(pkg):
    """two steps of the single-GPU ladder with the filter on: the last step's n_unique is the reference applied to the banks'
    forward list after DuplicateFiltering"""
    import torch
    w, h = 480, 360
    a, b, _ = synth.pair_partial(w, h)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    par = pkg.PairParams.default()
    ctx.set_local_affine(_par(pkg, PAIR_P))
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
    steps = [pkg.LadderStep.make((1,), 360.0), pkg.LadderStep.make((1, 2), 360.0)]
    pkg.ransac_pin_seed(7)
    res, _ = pkg.match_ladder_dev(ctx, dev.data_ptr(), w, h, steps, rep1, rep2, par, min_matches=10 ** 6)
    pkg.ransac_pin_seed(-1)
    counts = ctx.local_affine_counts()
    tent, u6, laf = pkg.match_reps(ctx, rep1, rep2)               # (mods_match_reps is not filtered)
    assert res.steps_done == 2 and res.n_tentatives == len(tent)
    tent, u6, laf = pkg.duplicate_filter(tent, u6, par.dup_dist, par.dup_mode, laf)
    ft = lr.filter_lists(tent, u6, laf, PAIR_P)[0]
    assert 0 < len(ft) < len(tent)
    assert res.n_unique == len(ft) and counts == (len(tent), len(ft))
    rep1.close(); rep2.close(); ctx.close()


def test_command_line(pkg, tmp_path):
    """one run of `mods` with [LocalAffineFiltering] on graf1 / graf6: its verbose counts are the library's"""
    import torch
    from PIL import Image
    import orc
    cfg = tmp_path / "la.ini"
    with open(os.path.join(CFG, "classic.ini")) as f:
        cfg.write_text(f.read() + "\n[LocalAffineFiltering]\ndoLocalAffineFiltering = 1\nradius = 160\nminSupport = 2\nkeepSparse = 0\n")
    env = dict(os.environ, MODS_RANSAC_SEED="4242")
    args = [MODS, G1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(cfg),
            os.path.join(CFG, "iters_one_view.ini")]
    p = subprocess.run(args, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    m = re.search(r"Local affine filtering \(radius 160\): (\d+) tentatives in, (\d+) kept", err)
    assert m, err
    cli_counts = (int(m.group(1)), int(m.group(2)))
    a, b = (orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB"))) for fn in (G1, G6))
    h, w = a.shape
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    ctx.set_local_affine(_par(pkg, dict(radius=160.0, minSupport=2, keepSparse=0)))
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(4242)
    res, _ = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0)], rep1, rep2, pkg.PairParams.default())
    pkg.ransac_pin_seed(-1)
    counts = ctx.local_affine_counts()
    rep1.close(); rep2.close(); ctx.close()
    assert cli_counts == counts and 0 < counts[1] < counts[0] and res.n_unique == counts[1]
    log = (tmp_path / "log.txt").read_text().split()
    assert len(log) == 7 and int(log[1]) == res.n_inliers and int(log[2]) == res.n_unique
