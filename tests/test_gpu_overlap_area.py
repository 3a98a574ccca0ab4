"""-m gpu: area-overlap matching (mods_match_overlap_area / mods_match_overlap_area_reps, csrc/overlap_area.hip) against the numpy
restatement of its contract (tests/overlap_area_ref.py).  Every case demands equality of q, t, the bits of E, the three lattice counts
and the counts of the call (the repeatability's bits included)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import overlap_area_ref as oar
import overlap_ref as orf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
H_PROJ = orf.H_PROJ
EYE = np.eye(3)
S10 = 10.0 / 3.0                  # 3 s = 10 exactly
SIZE = dict(w1=400, h1=300, w2=400, h2=300)


def assert_same(got, want, what=""):
    (gm, gc), (wm, wc) = got, want
    assert len(gm) == len(wm), (what, len(gm), len(wm))
    for f in ("q", "t", "n_q_px", "n_t_px", "n_both", "pad"):
        assert np.array_equal(gm[f], wm[f]), (what, f)
    assert np.array_equal(gm["E"].view(np.uint64), wm["E"].view(np.uint64)), (what, "E bits")
    assert (gc.n_q_common, gc.n_t_common, gc.n_matches) == (wc.n_q_common, wc.n_t_common, wc.n_matches), what
    assert np.float64(gc.repeatability).view(np.uint64) == np.float64(wc.repeatability).view(np.uint64), (what, "repeatability bits")
    assert gc.n_matches == len(gm)


def check_modes(pkg, ctx, q, t, H, what="", modes=(0, 1, 2), max_error=0.4, **size):
    """the library against the reference in the given modes; the evaluated pairs of the reference are formed once.  Returns the
    library's answers by mode and the reference's pair table"""
    pairs = oar.evaluated_pairs(q, t, oar.params(H, max_error, 0, **size))
    got = {}
    for mode in modes:
        got[mode] = ctx.match_overlap_area(q, t, pkg.OverlapAreaParams.default(H, max_error=max_error, one_to_one=mode, **size))
        assert_same(got[mode], oar.overlap_area_ref(q, t, oar.params(H, max_error, mode, **size), pairs), "%s mode %d" % (what, mode))
    return got, pairs


def _circles(rows, s=S10):
    rows = np.asarray(rows, np.float64).reshape(-1, 2)
    return orf.regions(rows, np.full(len(rows), s), np.tile(np.eye(2), (len(rows), 1, 1)))


@pytest.mark.parametrize("seed,n_q,n_t,least", [(7, 257, 131, 70), (11, 300, 301, 140), (3, 64, 65, 30)])
def test_scenes(pkg, gpu_ctx, seed, n_q, n_t, least):
    """list lengths around the 256-wide query blocks and train tiles, all three assignment modes; the reference alone finds enough
    matches, so an empty result cannot pass"""
    q, t = orf.scene(np.random.default_rng(seed), n_q, n_t)
    got, pairs = check_modes(pkg, gpu_ctx, q, t, H_PROJ, "seed %d" % seed)
    for mode in (0, 1, 2):
        assert len(oar.assign(pairs, 0.4, mode)) >= least
    assert len(got[2][0]) >= least and got[2][1].n_q_common == n_q and got[2][1].n_t_common == n_t
    assert len(got[0][0]) >= len(got[1][0]) and len(set(got[2][0]["t"].tolist())) == len(got[2][0])


def test_assignment_and_ties(pkg, gpu_ctx):
    q = _circles([(100, 100), (101.2, 100)])
    t = _circles([(101, 100), (103, 100)])
    got, _ = check_modes(pkg, gpu_ctx, q, t, EYE, "four regions")
    pairs_of = lambda m: list(zip(m["q"].tolist(), m["t"].tolist()))
    assert pairs_of(got[0][0]) == [(0, 0), (1, 0)] and pairs_of(got[1][0]) == [(1, 0)] and pairs_of(got[2][0]) == [(0, 1), (1, 0)]
    assert [tuple(int(v) for v in (r["n_q_px"], r["n_t_px"], r["n_both"])) for r in got[2][0]] == [(2821, 2821, 2288), (2818, 2821, 2784)]
    # identical circles: E = +0.0 exactly
    got, _ = check_modes(pkg, gpu_ctx, q[:1], _circles([(100, 100)]), EYE, "identical")
    assert got[2][0]["E"].view(np.uint64).tolist() == [0] and got[2][0]["n_both"].tolist() == [2821]
    # two identical trains: the lower index, whatever their places; also across two train tiles and (with splits) two splits
    for mode_t in ([(101, 100), (101, 100)], [(300, 300), (101, 100), (300, 20), (101, 100)]):
        got, _ = check_modes(pkg, gpu_ctx, q[:1], _circles(mode_t), EYE, "twins")
        first = mode_t.index((101, 100))
        assert all(got[m][0]["t"].tolist() == [first] for m in (0, 1, 2))
    far = _circles(np.full((600, 2), 300.0))
    far[[255, 256, 599]] = _circles([(101, 100)])[0]
    far["id"] = np.arange(600)
    got, _ = check_modes(pkg, gpu_ctx, q[:1], far, EYE, "twins over tiles")
    assert all(got[m][0]["t"].tolist() == [255] for m in (0, 1, 2))
    # two queries with equal errors on one train: the lower query owns it (modes 1 and 2)
    q2 = _circles([(100.5, 100), (99.5, 100), (100, 100.25)])
    got, _ = check_modes(pkg, gpu_ctx, q2, _circles([(100, 100)]), EYE, "one train")
    assert got[0][0]["q"].tolist() == [0, 1, 2] and got[0][0]["E"][0] == got[0][0]["E"][1] > got[0][0]["E"][2]
    assert got[1][0]["q"].tolist() == [2] and got[2][0]["q"].tolist() == [2]
    got, _ = check_modes(pkg, gpu_ctx, q2[:2], _circles([(100, 100)]), EYE, "one train, a tie")
    assert got[1][0]["q"].tolist() == [0] and got[2][0]["q"].tolist() == [0]


@pytest.mark.parametrize("n_q,n_t", [(1, 1), (0, 5), (5, 0), (0, 0)])
def test_tails(pkg, gpu_ctx, n_q, n_t):
    q, t = orf.scene(np.random.default_rng(21), max(n_q, 1), max(n_t, 1))
    q["x"][0], q["y"][0] = 200.0, 150.0                                # well inside both images
    J, p = orf.lin_h(H_PROJ, np.c_[q["x"][:1], q["y"][:1]])
    t[0] = orf.regions(p, [q["s"][0]], J @ np.array([[q["a11"][0], q["a12"][0]], [q["a21"][0], q["a22"][0]]]))[0]   # the exact image of q[0]
    got, _ = check_modes(pkg, gpu_ctx, q[:n_q], t[:n_t], H_PROJ, "%d x %d" % (n_q, n_t), **SIZE)
    for m in (0, 1, 2):
        assert len(got[m][0]) == min(n_q, n_t, 1)
        assert got[m][1].n_q_common <= n_q and got[m][1].n_t_common <= n_t
    if n_q and n_t:
        assert got[2][0]["E"][0] < 0.01 and got[2][1].repeatability == 1.0


def test_common_area(pkg, gpu_ctx):
    """image sizes on and off: with them regions outside the common area neither match nor count"""
    q, t = orf.scene(np.random.default_rng(9), 200, 180, w=520.0, h=390.0)
    p_on = oar.params(H_PROJ, **SIZE)
    mq, mt = orf.common_masks(q, t, p_on)
    assert 20 < mq.sum() < len(q) - 20 and 20 < mt.sum() < len(t) - 20
    on, _ = check_modes(pkg, gpu_ctx, q, t, H_PROJ, "sizes on", **SIZE)
    off, _ = check_modes(pkg, gpu_ctx, q, t, H_PROJ, "sizes off")
    for m in (0, 1, 2):
        assert (on[m][1].n_q_common, on[m][1].n_t_common) == (int(mq.sum()), int(mt.sum()))
        assert (off[m][1].n_q_common, off[m][1].n_t_common) == (len(q), len(t))
        assert mq[on[m][0]["q"]].all() and mt[on[m][0]["t"]].all() and 10 < len(on[m][0]) < len(off[m][0])
        assert 0 < on[m][1].repeatability <= 1
    one, _ = check_modes(pkg, gpu_ctx, q, t, H_PROJ, "one size missing", modes=(2,), w1=400, h1=300, w2=0, h2=300)
    assert one[2][1].n_q_common == len(q)
    # image sizes that leave no region in the area: repeatability 0
    none, _ = check_modes(pkg, gpu_ctx, q, t, np.array([[1, 0, 5000], [0, 1, 0], [0, 0, 1.0]]), "nothing in common", modes=(2,), **SIZE)
    assert len(none[2][0]) == 0 and (none[2][1].n_q_common, none[2][1].n_t_common, none[2][1].repeatability) == (0, 0, 0.0)


def test_gates_and_cap(pkg, gpu_ctx):
    """the cases of tests/test_cpu_overlap_area.py::test_gates in one pair of lists, far enough apart not to meet each other"""
    frames = [np.diag([8.0, 1.0 / 8.0]), np.diag([9.0, 1.0 / 9.0]), np.diag([1.0 / 9.0, 9.0])] + [np.eye(2)] * 9
    tframes = frames[:3] + [np.eye(2) * np.sqrt(r) for r in (0.48, 0.53, 0.55, 1.8, 1.9)] + [np.eye(2)] * 4
    qxy = np.array([(300.0 + 700.0 * i, 500.0) for i in range(12)])
    txy = qxy.copy()
    txy[8] += (20, 0); txy[9] += (20.01, 0); txy[10] += (0, -20.1); txy[11] += (3, 1)
    q = orf.regions(qxy, np.full(12, S10), frames)
    t = orf.regions(txy, np.full(12, S10), tframes)
    got, pairs = check_modes(pkg, gpu_ctx, q, t, EYE, "gates")
    ev = list(zip(pairs["q"].tolist(), pairs["t"].tolist()))
    assert ev == [(0, 0), (5, 5), (6, 6), (8, 8), (11, 11)]
    assert got[2][0]["q"].tolist() == [0, 11] and got[2][0]["E"][0] == 0.0 and got[2][0]["n_both"][0] > 2000
    # max_error = 1 opens the area gate; 0.5 moves it to 0.45
    got, pairs = check_modes(pkg, gpu_ctx, q, t, EYE, "gates, max_error 1", max_error=1.0)
    assert len(pairs) == 8 and got[0][0]["q"].tolist() == [0, 3, 4, 5, 6, 7, 8, 11]
    got, pairs = check_modes(pkg, gpu_ctx, q, t, EYE, "gates, max_error 0.5", modes=(2,), max_error=0.5)
    assert len(pairs) == 8 and got[2][0]["q"].tolist() == [0, 4, 5, 6, 7, 11]


def test_degenerate_records(pkg, gpu_ctx):
    """trains with an all-zero frame or s = 0, queries on the line den == 0, NaN and infinite fields: never matched, never a fault, and
    their neighbours keep their matches"""
    rng = np.random.default_rng(5)
    Hs = np.array([[1, 0, 0], [0, 1, 0], [1.0 / 256, 0, -1.0]])      # den = x / 256 - 1: exactly zero on x = 256
    for H in (H_PROJ, Hs):
        size = SIZE if H is H_PROJ else {}
        q, t = orf.scene(rng, 220, 200, H)
        clean = oar.overlap_area_ref(q, t, oar.params(H, 0.4, 0, **size))[0]
        q["x"][:20] = 256.0
        q["y"][20:25] = np.nan; q["s"][25:30] = np.inf; q["a12"][30:33] = -np.inf
        for f in ("a11", "a12", "a21", "a22"):
            t[f][:15] = 0.0
        t["s"][15:30] = 0.0
        t["x"][30:35] = np.nan; t["a21"][35:38] = np.nan; t["s"][38:40] = -np.inf
        got, _ = check_modes(pkg, gpu_ctx, q, t, H, "degenerate", **size)
        for m in (0, 1, 2):
            assert len(got[m][0]) > 10
            assert not np.isin(got[m][0]["q"], np.arange(20, 33)).any() and not np.isin(got[m][0]["t"], np.arange(40)).any()
            if H is Hs:
                assert not np.isin(got[m][0]["q"], np.arange(20)).any()
        # a query whose partner was not touched keeps it
        keep = clean[(clean["q"] >= 33) & (clean["t"] >= 40)]
        have = set(zip(got[0][0]["q"].tolist(), got[0][0]["t"].tolist()))
        assert len(keep) > 10 and all(k in have for k in zip(keep["q"].tolist(), keep["t"].tolist()))
    got, _ = check_modes(pkg, gpu_ctx, q, t[:30], H_PROJ, "only degenerate trains")
    assert len(got[2][0]) == 0 and (got[2][1].n_q_common, got[2][1].n_t_common, got[2][1].repeatability) == (220, 30, 0.0)
    # max_error = 1 opens the area gate: trains of no area are walked, count nothing and match nothing
    q1 = _circles([(100, 100), (140, 100)])
    t1 = np.r_[orf.regions([(100, 100), (140, 100)], [S10, 0.0], [np.zeros((2, 2)), np.eye(2)]),
               orf.regions([(100, 100)], [S10], [np.array([[1.0, 2.0], [2.0, 4.0]])]), _circles([(141, 100)])]
    got, pairs = check_modes(pkg, gpu_ctx, q1, t1, EYE, "no area", max_error=1.0)
    assert len(pairs) >= 4 and (pairs["n_t_px"][pairs["t"] < 3] == 0).all()
    assert all(list(zip(got[m][0]["q"].tolist(), got[m][0]["t"].tolist())) == [(1, 3)] for m in (0, 1, 2))


@pytest.fixture(scope="module")
def big(pkg):
    """a scene of several query blocks and train tiles and its reference, shared by the tests below"""
    q, t = orf.scene(np.random.default_rng(37), 700, 1100, w=900.0, h=700.0)
    size = dict(w1=900, h1=700, w2=900, h2=700)
    pairs = oar.evaluated_pairs(q, t, oar.params(H_PROJ, 0.4, 0, **size))
    want = {m: oar.overlap_area_ref(q, t, oar.params(H_PROJ, 0.4, m, **size), pairs) for m in (0, 1, 2)}
    assert len(want[2][0]) > 100
    return q, t, size, want


def test_launch_independence(pkg, gpu_ctx, big):
    """one train split, three, seven, more splits than tiles and the automatic choice: one answer, also when repeated"""
    q, t, size, want = big
    try:
        for splits in (0, 1, 3, 7, 1000):
            gpu_ctx.overlap_splits(splits)
            for m in (0, 1, 2):
                p = pkg.OverlapAreaParams.default(H_PROJ, one_to_one=m, **size)
                assert_same(gpu_ctx.match_overlap_area(q, t, p), want[m], "splits %d mode %d" % (splits, m))
            assert_same(gpu_ctx.match_overlap_area(q, t, p), want[2], "splits %d, repeated" % splits)
    finally:
        gpu_ctx.overlap_splits(0)


def test_banks_capacity_and_neighbours(pkg, gpu_ctx, big):
    q, t, size, want = big
    rng = np.random.default_rng(2)
    q = q.copy(); t = t.copy()
    q["desc"] = rng.integers(0, 256, (len(q), 128), dtype=np.uint8); t["desc"] = rng.integers(0, 256, (len(t), 128), dtype=np.uint8)
    t["desc"][:200] = q["desc"][:200]                                  # (tentatives for the FGINN search below)
    rq, rt = pkg.ImgRep(gpu_ctx, 4096), pkg.ImgRep(gpu_ctx, 4096)
    try:
        rq.append_host(q[:300]); rq.append_host(q[300:]); rt.append_host(t)
        for m in (0, 1, 2):
            p = pkg.OverlapAreaParams.default(H_PROJ, one_to_one=m, **size)
            bank = pkg.match_overlap_area_reps(gpu_ctx, rq, rt, p)
            assert_same(bank, want[m], "banks vs reference, mode %d" % m)
            assert_same(bank, gpu_ctx.match_overlap_area(q, t, p), "banks vs host lists, mode %d" % m)
            # a result longer than the room given: the full length, MODS_E_CAPACITY, the counts filled, nothing copied
            n_full = len(bank[0])
            with pytest.raises(pkg.ModsError, match="overflow"):
                pkg.match_overlap_area_reps(gpu_ctx, rq, rt, p, cap=n_full - 1)
            out = np.full(n_full, 7, pkg.OVERLAP_AREA_DTYPE)
            n = C.c_int(-1)
            counts = pkg.OverlapCounts()
            for call in (lambda: pkg.lib().mods_match_overlap_area_reps(gpu_ctx.h, rq.h, rt.h, C.byref(p), out.ctypes.data_as(C.c_void_p), n_full - 1,
                                                                        C.byref(n), C.byref(counts)),
                         lambda: pkg.lib().mods_match_overlap_area(gpu_ctx.h, q.ctypes.data_as(C.c_void_p), len(q), t.ctypes.data_as(C.c_void_p),
                                                                   len(t), C.byref(p), None, 0, C.byref(n), C.byref(counts))):
                n.value = -1
                assert call() == -3 and n.value == n_full and counts.n_matches == n_full
                assert (counts.n_q_common, counts.n_t_common) == (bank[1].n_q_common, bank[1].n_t_common)
                assert pkg.lib().mods_last_error().startswith(b"match_overlap_area: ")
                assert (out["q"] == 7).all() and (out["E"] == 7).all()
            assert_same(pkg.match_overlap_area_reps(gpu_ctx, rq, rt, p, cap=n_full), want[m], "after the overflow")
        # the matcher's "last search" and the linearised overlap search are left alone by a call in between
        tent, u6 = gpu_ctx.match_fginn(q, t, 0.9)
        assert len(tent) > 0
        lp = pkg.OverlapParams.default(H_PROJ, **size)
        lin = gpu_ctx.match_overlap(q, t, lp)
        assert_same(pkg.match_overlap_area_reps(gpu_ctx, rq, rt, p), want[2], "behind the other searches")
        cap = len(q)
        tent2 = np.zeros(cap, pkg.TENT_DTYPE); u62 = np.zeros((cap, 6)); laf2 = np.zeros((cap, 14))
        n = C.c_int(-1)
        assert pkg.lib().mods_match_fetch_internal(gpu_ctx.h, tent2.ctypes.data_as(C.c_void_p), u62.ctypes.data_as(C.c_void_p),
                                                   laf2.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
        assert n.value == len(tent) and tent2[:n.value].tobytes() == tent.tobytes() and np.array_equal(u62[:n.value], u6)
        lin2 = gpu_ctx.match_overlap(q, t, lp)
        assert len(lin[0]) > 10 and lin2[0].tobytes() == lin[0].tobytes() and lin2[1].n_matches == lin[1].n_matches
    finally:
        rq.close(); rt.close()


def test_stage_timer(pkg, gpu_ctx, big):
    """the stage reports its launches: two scopes per search, the host reads the list length between them"""
    q, t, size, want = big
    p = pkg.OverlapAreaParams.default(H_PROJ, **size)
    try:
        gpu_ctx.timing_enable(["overlap_area", "overlap"]); gpu_ctx.timing_reset()
        for _ in range(3):
            assert_same(gpu_ctx.match_overlap_area(q, t, p), want[2], "timed")
        ms, launches, by = gpu_ctx.timing_read("overlap_area")
        assert launches == 6 and ms > 0 and by == 3.0 * (len(q) + len(t)) * q.dtype.itemsize
        assert gpu_ctx.timing_read("overlap")[1] == 0
    finally:
        gpu_ctx.timing_enable([]); gpu_ctx.timing_reset()


def _grey(fn):
    import orc
    from PIL import Image
    return orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB")))


def _npz_regions(fn):
    z = np.load(fn)
    n = len(z["xy"])
    r = np.zeros(n, orf.REGION_DTYPE)
    r["x"], r["y"] = z["xy"].T
    r["s"] = z["scales"][:, 0]
    r["a11"], r["a12"], r["a21"], r["a22"] = z["A"].T
    return r


def test_cli_area_overlap(pkg, gpu_ctx, tmp_path):
    """ver_type 1 with the ground-truth homography and overlapMeasure = area: the new stderr line with the count the API gives on
    the regions the same run wrote (equal to the reference's); the matches file and the log row are those of a run with linear"""
    import torch
    a, b = _grey(G1), _grey(G6)
    h, w = a.shape
    img = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(4242)
    try:
        res, _ = pkg.match_pair_dev(gpu_ctx, img.data_ptr(), w, h, pkg.PairParams.default())
    finally:
        pkg.ransac_pin_seed(-1)
    assert res.n_inliers >= 15
    H = np.array(list(res.H))                                          # the homography the existing overlap CLI test uses
    ini = open(os.path.join(CFG, "classic.ini")).read()
    (tmp_path / "a.ini").write_text(ini + "\n[OverlapMatching]\ndoOverlapMatch = 1\noverlapMeasure = area\n")
    (tmp_path / "l.ini").write_text(ini + "\n[OverlapMatching]\ndoOverlapMatch = 1\noverlapMeasure = linear\n")
    (tmp_path / "H.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in H.reshape(3, 3)) + "\n")
    env = dict(os.environ, MODS_RANSAC_SEED="4242")

    def run(config, tag):
        args = [MODS, G1, G6, "o1.png", "o2.png", "k1%s.npz" % tag, "k2%s.npz" % tag, "m%s.txt" % tag, "log%s.txt" % tag, "0", "1", "H.txt",
                config, os.path.join(CFG, "iters_one_view.ini")]
        p = subprocess.run(args, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        return p.stderr.decode()

    err = run(str(tmp_path / "a.ini"), "a")
    lines = err.splitlines()
    at = lines.index("Area overlap matches with error < 0.4")
    n_cli = int(lines[at + 1])
    assert "Overlap matches with E <" not in err
    r1, r2 = _npz_regions(tmp_path / "k1a.npz"), _npz_regions(tmp_path / "k2a.npz")
    kw = dict(max_error=0.4, one_to_one=2, w1=w, h1=h, w2=w, h2=h)
    m, c = gpu_ctx.match_overlap_area(r1, r2, pkg.OverlapAreaParams.default(H, **kw))
    assert n_cli == c.n_matches > 0
    assert "HessianAffine: %d | %d regions in the common area, repeatability " % (c.n_q_common, c.n_t_common) in err      # verbose = 1
    assert_same((m, c), oar.overlap_area_ref(r1, r2, oar.params(H, **kw)), "graf")
    err_l = run(str(tmp_path / "l.ini"), "l")
    assert "Overlap matches with E < 0.09" in err_l and "Area overlap" not in err_l
    assert (tmp_path / "ml.txt").read_bytes() == (tmp_path / "ma.txt").read_bytes()
    la, ll = (tmp_path / "loga.txt").read_text().split(), (tmp_path / "logl.txt").read_text().split()
    assert len(la) == len(ll) == 10 and la[1:] == ll[1:]              # (the first field is the run time)
    print("graf1/graf6 one view: %d | %d regions, %d | %d in the common area, area overlap matches (error < 0.4, greedy) %d, repeatability %.4f"
          % (len(r1), len(r2), c.n_q_common, c.n_t_common, c.n_matches, c.repeatability))
