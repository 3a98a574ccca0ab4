"""-m gpu: overlap matching (mods_match_overlap / mods_match_overlap_reps, csrc/overlap.hip) against the numpy restatement of its
contract (tests/overlap_ref.py).  Every case demands equality to the bit of q, t, the bits of E, dist and diff, and the counts
(the repeatability's bits included)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import overlap_ref as orf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
H_PROJ = orf.H_PROJ
EYE = np.eye(3)
S4 = 4.0 / 3.0                    # 3 s = 4 exactly


def assert_same(got, want, what=""):
    (gm, gc), (wm, wc) = got, want
    assert len(gm) == len(wm), (what, len(gm), len(wm))
    for f in ("q", "t"):
        assert np.array_equal(gm[f], wm[f]), (what, f)
    for f in ("E", "dist", "diff"):
        assert np.array_equal(gm[f].view(np.uint64), wm[f].view(np.uint64)), (what, f + " bits")
    assert (gc.n_q_common, gc.n_t_common, gc.n_matches) == (wc.n_q_common, wc.n_t_common, wc.n_matches), what
    assert np.float64(gc.repeatability).view(np.uint64) == np.float64(wc.repeatability).view(np.uint64), (what, "repeatability bits")
    assert gc.n_matches == len(gm)


def check(pkg, ctx, q, t, H, what="", **kw):
    got = ctx.match_overlap(q, t, pkg.OverlapParams.default(H, **kw))
    assert_same(got, orf.overlap_ref(q, t, orf.params(H, **kw)), what)
    return got


@pytest.mark.parametrize("n_q,n_t", [(0, 5), (5, 0), (1, 1), (63, 65), (300, 257), (5000, 4099)])
@pytest.mark.parametrize("oriented", [1, 0])
def test_list_lengths(pkg, gpu_ctx, n_q, n_t, oriented):
    """list lengths around the 256-wide query blocks and train tiles; (5000, 4099) spans 20 query blocks and several train splits.
    The oriented cases run with the common-area test, the others without it"""
    rng = np.random.default_rng(100 + n_q + n_t)
    q, t = orf.scene(rng, n_q, n_t)
    size = dict(w1=400, h1=300, w2=400, h2=300) if oriented else {}
    m, c = check(pkg, gpu_ctx, q, t, H_PROJ, oriented=oriented, one_to_one=n_q % 2, **size)
    if n_q >= 300:
        assert len(m) > 10 and n_q - len(m) > 10
    if not size:
        assert (c.n_q_common, c.n_t_common) == (n_q, n_t)
    if (n_q, n_t) == (1, 1):
        J, p = orf.lin_h(H_PROJ, np.array([[50.0, 60.0]]))
        q1 = orf.regions([(50.0, 60.0)], [2.0], [np.eye(2)])
        t1 = orf.regions(p, [2.0], J)                                # the exact image of q1: E is rounding noise
        m, c = check(pkg, gpu_ctx, q1, t1, H_PROJ, oriented=oriented)
        assert len(m) == 1 and m["E"][0] < 1e-20 and c.repeatability == 1.0


def test_decision_boundary(pkg, gpu_ctx):
    """max_error at a pair's own E rejects it (E1 < max_error is strict), the next double accepts it"""
    rng = np.random.default_rng(3)
    q, t = orf.scene(rng, 300, 257)
    for oriented in (1, 0):
        base, _ = check(pkg, gpu_ctx, q, t, H_PROJ, oriented=oriented, one_to_one=0)
        assert len(base) > 10
        for row in base[[0, len(base) // 2, -1]]:
            e = float(row["E"])
            lo, _ = check(pkg, gpu_ctx, q, t, H_PROJ, max_error=e, oriented=oriented, one_to_one=0)
            assert row["q"] not in lo["q"]
            hi, _ = check(pkg, gpu_ctx, q, t, H_PROJ, max_error=float(np.nextafter(e, np.inf)), oriented=oriented, one_to_one=0)
            k = np.nonzero(hi["q"] == row["q"])[0]
            assert len(k) == 1 and hi["t"][k[0]] == row["t"] and hi["E"][k[0]] == e


def test_ties_one_to_one_and_orientation(pkg, gpu_ctx):
    ident = np.eye(2)
    # two identical trains: the lower index; the same pair in the other order of the list
    q = orf.regions([(50, 50)], [S4], [ident])
    t = orf.regions([(90, 90), (50.5, 50), (50.5, 50), (50.25, 50)], [S4, S4, S4, 2 * S4], [ident] * 4)
    m, _ = check(pkg, gpu_ctx, q, t, EYE, one_to_one=0)
    assert m["t"].tolist() == [1] and m["E"].tolist() == [0.015625]         # train 3 is nearer (dist 1/1024) but half the size: diff 0.25
    m, _ = check(pkg, gpu_ctx, q, t[::-1].copy(), EYE, one_to_one=0)
    assert m["t"].tolist() == [1]
    # a tie that straddles two train tiles and (with 2 splits) two splits: still the lower index
    far = orf.regions(np.full((600, 2), 500.0), np.full(600, S4), [ident] * 600)
    tt = far.copy(); tt[[255, 256, 599]] = t[1]
    m, _ = check(pkg, gpu_ctx, q, tt, EYE, one_to_one=0)
    assert m["t"].tolist() == [255]
    # two queries on one train
    q2 = orf.regions([(50, 50), (51, 50), (50.5, 50.5), (50.5, 49.5)], [S4] * 4, [ident] * 4)
    t2 = orf.regions([(50.5, 50)], [S4], [ident])
    m, c = check(pkg, gpu_ctx, q2, t2, EYE, one_to_one=0)
    assert m["q"].tolist() == [0, 1, 2, 3] and len(set(m["E"].tolist())) == 1
    m, c = check(pkg, gpu_ctx, q2, t2, EYE, one_to_one=1)
    assert m["q"].tolist() == [0] and c.n_matches == 1                       # equal errors: the lowest query owns the train
    q2["x"][2] = 50.25; q2["y"][2] = 50.0
    m, c = check(pkg, gpu_ctx, q2, t2, EYE, one_to_one=1)
    assert m["q"].tolist() == [2]                                            # the smaller error wins over the lower index
    # a copy rotated in the plane of the frame: the same ellipse, another orientation
    th = 1.1
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    A = np.array([[1.3, 0.0], [0.4, 1 / 1.3]])
    q3 = orf.regions([(70, 80)], [3.0], [A])
    t3 = orf.regions([(70, 80)], [3.0], [A @ R])
    assert len(check(pkg, gpu_ctx, q3, t3, EYE, oriented=1)[0]) == 0
    m, _ = check(pkg, gpu_ctx, q3, t3, EYE, oriented=0)
    assert len(m) == 1 and m["E"][0] < 1e-20


def test_degenerate_records(pkg, gpu_ctx):
    """a train with an all-zero frame, one with s = 0, a query on the line den == 0, NaN coordinates: never matched, never a fault,
    and their neighbours keep their matches"""
    rng = np.random.default_rng(5)
    Hs = np.array([[1, 0, 0], [0, 1, 0], [1.0 / 256, 0, -1.0]])      # den = x / 256 - 1: exactly zero on x = 256
    for H in (H_PROJ, Hs):
        q, t = orf.scene(rng, 700, 600, H)
        clean = orf.overlap_ref(q, t, orf.params(H, one_to_one=0))[0]
        q["x"][:40] = 256.0
        q["y"][40:50] = np.nan; q["s"][50:55] = np.inf
        for f in ("a11", "a12", "a21", "a22"):
            t[f][:30] = 0.0
        t["s"][30:60] = 0.0
        t["x"][60:70] = np.nan; t["a21"][70:75] = np.nan; t["s"][75:80] = -np.inf
        for oriented in (1, 0):
            for size in ({}, dict(w1=400, h1=300, w2=400, h2=300)) if H is H_PROJ else ({},):
                m, c = check(pkg, gpu_ctx, q, t, H, oriented=oriented, one_to_one=0, **size)
                assert len(m) > 10
                assert not np.isin(m["q"], np.arange(40, 55)).any() and not np.isin(m["t"], np.arange(80)).any()
                if H is Hs:
                    assert not np.isin(m["q"], np.arange(40)).any()
        m, _ = check(pkg, gpu_ctx, q, t, H, one_to_one=0)
        # a query whose partner was not touched keeps it
        keep = clean[(clean["q"] >= 55) & (clean["t"] >= 80)]
        have = set(zip(m["q"].tolist(), m["t"].tolist()))
        assert len(keep) > 10 and all(k in have for k in zip(keep["q"].tolist(), keep["t"].tolist()))
    # only degenerate trains: nothing, and the counts stand
    m, c = check(pkg, gpu_ctx, q, t[:60], H_PROJ, one_to_one=1)
    assert len(m) == 0 and (c.n_q_common, c.n_t_common, c.repeatability) == (700, 60, 0.0)


def test_common_area(pkg, gpu_ctx):
    """H = the translation by (3, 4), so every border can be hit exactly: px == 0 and px == w2, py == 0 and py == h2, and the same for
    the trains sent back.  Both inequalities are strict"""
    H = np.array([[1, 0, 3], [0, 1, 4], [0, 0, 1.0]])
    w1, h1, w2, h2 = 120, 90, 110, 100
    ident = np.eye(2)
    qxy = [(-3, 20), (107, 20), (20, -4), (20, 96), (-2.75, 20), (106.75, 20), (20, -3.75), (20, 95.75), (50, 50), (-40, 50), (50, 300)]
    txy = [(3, 30), (123, 30), (30, 4), (30, 94), (3.25, 30), (122.75, 30), (30, 4.25), (30, 93.75), (53, 54), (109.75, 24), (400, 30)]
    rng = np.random.default_rng(9)
    q0, t0 = orf.scene(rng, 200, 180, H, w=130.0, h=110.0)
    q = np.r_[orf.regions(qxy, [S4] * len(qxy), [ident] * len(qxy)), q0]
    t = np.r_[orf.regions(txy, [S4] * len(txy), [ident] * len(txy)), t0]
    mq, mt = orf.common_masks(q, t, orf.params(H, w1=w1, h1=h1, w2=w2, h2=h2))
    assert mq[:11].tolist() == [False] * 4 + [True] * 5 + [False] * 2
    assert mt[:11].tolist() == [False] * 4 + [True] * 6 + [False]
    assert 20 < mq.sum() < len(q) - 20 and 20 < mt.sum() < len(t) - 20
    for kw in (dict(one_to_one=1), dict(one_to_one=0, oriented=0), dict(one_to_one=1, max_error=0.5)):
        m, c = check(pkg, gpu_ctx, q, t, H, str(kw), w1=w1, h1=h1, w2=w2, h2=h2, **kw)
        assert (c.n_q_common, c.n_t_common) == (int(mq.sum()), int(mt.sum())) and 0 < c.repeatability < 1
        assert mq[m["q"]].all() and mt[m["t"]].all()
        assert 8 in m["q"] and m["t"][m["q"] == 8].tolist() == [8]          # (50, 50) -> (53, 54)
        assert 5 in m["q"] and m["t"][m["q"] == 5].tolist() == [9]          # (106.75, 20) -> (109.75, 24): just inside both
    # one size missing: no test, every region takes part
    m, c = check(pkg, gpu_ctx, q, t, H, w1=w1, h1=h1, w2=0, h2=h2)
    assert (c.n_q_common, c.n_t_common) == (len(q), len(t)) and not mq[m["q"]].all()
    # image sizes that leave one list without a region in the area: repeatability 0
    m, c = check(pkg, gpu_ctx, q, t, np.array([[1, 0, 5000], [0, 1, 0], [0, 0, 1.0]]), w1=w1, h1=h1, w2=w2, h2=h2)
    assert len(m) == 0 and (c.n_q_common, c.n_t_common, c.repeatability) == (0, 0, 0.0)


def test_launch_independence(pkg, gpu_ctx):
    """the same lists with one train split, three, more splits than tiles and the automatic choice: one answer; and with the trains
    in reverse order, mapped back, the same answer wherever no two trains of a query tie"""
    rng = np.random.default_rng(37)
    q, t = orf.scene(rng, 3000, 2100)
    for oriented in (1, 0):
        p = pkg.OverlapParams.default(H_PROJ, oriented=oriented, one_to_one=1, w1=400, h1=300, w2=400, h2=300)
        want = orf.overlap_ref(q, t, orf.params(H_PROJ, oriented=oriented, one_to_one=1, w1=400, h1=300, w2=400, h2=300))
        try:
            for splits in (1, 3, 1000, 0):
                gpu_ctx.overlap_splits(splits)
                assert_same(gpu_ctx.match_overlap(q, t, p), want, "splits %d" % splits)
                assert_same(gpu_ctx.match_overlap(q, t, p), want, "splits %d, repeated" % splits)
        finally:
            gpu_ctx.overlap_splits(0)
        rev = gpu_ctx.match_overlap(q, t[::-1].copy(), p)
        assert np.array_equal(rev[0]["q"], want[0]["q"]) and np.array_equal(len(t) - 1 - rev[0]["t"], want[0]["t"])
        assert np.array_equal(rev[0]["E"], want[0]["E"])


def test_banks_equal_host_lists_and_capacity(pkg, gpu_ctx):
    rng = np.random.default_rng(41)
    q, t = orf.scene(rng, 1300, 1100)
    rq, rt = pkg.ImgRep(gpu_ctx, 4096), pkg.ImgRep(gpu_ctx, 4096)
    try:
        rq.append_host(q[:700]); rq.append_host(q[700:]); rt.append_host(t)
        for kw in (dict(one_to_one=0), dict(one_to_one=1, oriented=0, w1=400, h1=300, w2=400, h2=300)):
            p = pkg.OverlapParams.default(H_PROJ, **kw)
            host = gpu_ctx.match_overlap(q, t, p)
            bank = pkg.match_overlap_reps(gpu_ctx, rq, rt, p)
            assert len(host[0]) > 100
            assert_same(bank, host, "banks")
            assert_same(bank, orf.overlap_ref(q, t, orf.params(H_PROJ, **kw)), "banks vs reference")
        # a result longer than the room given: the full length, MODS_E_CAPACITY, nothing copied - as mods_match_guided answers
        n_full = len(host[0])
        with pytest.raises(pkg.ModsError, match="overflow"):
            pkg.match_overlap_reps(gpu_ctx, rq, rt, p, cap=n_full - 1)
        out = np.full(n_full, 7, pkg.OVERLAP_DTYPE)
        n = C.c_int(-1)
        counts = pkg.OverlapCounts()
        for call in (lambda: pkg.lib().mods_match_overlap_reps(gpu_ctx.h, rq.h, rt.h, C.byref(p), out.ctypes.data_as(C.c_void_p), n_full - 1,
                                                               C.byref(n), C.byref(counts)),
                     lambda: pkg.lib().mods_match_overlap(gpu_ctx.h, q.ctypes.data_as(C.c_void_p), len(q), t.ctypes.data_as(C.c_void_p), len(t),
                                                          C.byref(p), None, 0, C.byref(n), C.byref(counts))):
            n.value = -1
            assert call() == -3 and n.value == n_full and counts.n_matches == n_full
            assert pkg.lib().mods_last_error().startswith(b"match_overlap: ")
            assert (out["q"] == 7).all() and (out["E"] == 7).all()
        # afterwards the context still works
        assert_same(pkg.match_overlap_reps(gpu_ctx, rq, rt, p, cap=n_full), host, "after the overflow")
    finally:
        rq.close(); rt.close()


def _grey(fn):
    import orc
    from PIL import Image
    return orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB")))


@pytest.fixture(scope="module")
def graf(pkg, gpu_ctx):
    """graf1 / graf6 through the pair entry point (one view): the verified homography and the context's regions"""
    import torch
    a, b = _grey(G1), _grey(G6)
    h, w = a.shape
    assert (w, h) == (800, 640)
    img = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(4242)
    try:
        res, _ = pkg.match_pair_dev(gpu_ctx, img.data_ptr(), w, h, pkg.PairParams.default())
    finally:
        pkg.ransac_pin_seed(-1)
    assert res.n_inliers >= 15
    return np.array(list(res.H)), gpu_ctx.regions_fetch(0), gpu_ctx.regions_fetch(1), res.n_inliers


def test_end_to_end_graf(pkg, gpu_ctx, graf, capsys):
    """the context's regions into banks, overlap matching on them under the pair's verified homography: equal to the reference on
    the fetched regions.  The counts are printed (profiles/overlap_timing.txt records them), not compared."""
    H, r1, r2, n_inliers = graf
    rq, rt = pkg.ImgRep(gpu_ctx, len(r1) + 1), pkg.ImgRep(gpu_ctx, len(r2) + 1)
    try:
        rq.append_ctx(0); rt.append_ctx(1)
        kw = dict(max_error=0.09, one_to_one=1, w1=800, h1=640, w2=800, h2=640)
        got = pkg.match_overlap_reps(gpu_ctx, rq, rt, pkg.OverlapParams.default(H, **kw))
        assert_same(got, orf.overlap_ref(r1, r2, orf.params(H, **kw)), "graf")
        c = got[1]
        assert 0 < c.n_matches <= min(c.n_q_common, c.n_t_common)
        un = pkg.match_overlap_reps(gpu_ctx, rq, rt, pkg.OverlapParams.default(H, oriented=0, **kw))
        assert_same(un, orf.overlap_ref(r1, r2, orf.params(H, oriented=0, **kw)), "graf, unoriented")
        with capsys.disabled():
            print("\ngraf1/graf6 one view: regions %d | %d, RANSAC inliers %d, in the common area %d | %d, overlap matches (E < 0.09, one to "
                  "one) %d oriented (repeatability %.4f), %d unoriented (repeatability %.4f)"
                  % (len(r1), len(r2), n_inliers, c.n_q_common, c.n_t_common, c.n_matches, c.repeatability, un[1].n_matches,
                     un[1].repeatability))
    finally:
        rq.close(); rt.close()


def _npz_regions(fn):
    z = np.load(fn)
    n = len(z["xy"])
    r = np.zeros(n, orf.REGION_DTYPE)
    r["x"], r["y"] = z["xy"].T
    r["s"] = z["scales"][:, 0]
    r["a11"], r["a12"], r["a21"], r["a22"] = z["A"].T
    return r


def test_cli_overlap(pkg, gpu_ctx, graf, tmp_path):
    """ver_type 1 with the homography as the ground-truth file and [OverlapMatching] doOverlapMatch = 1: the two stderr lines of
    mods.cpp:522-523 with the count the API gives on the regions the same run wrote; doOverlapMatch = 0: no word of it anywhere, and
    the matches file and the log row are those of the run with the key"""
    H = graf[0]
    ini = open(os.path.join(CFG, "classic.ini")).read()
    (tmp_path / "c.ini").write_text(ini + "\n[OverlapMatching]\ndoOverlapMatch = 1\n")
    env = dict(os.environ, MODS_RANSAC_SEED="4242")

    def run(config, tag):
        (tmp_path / "H.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in H.reshape(3, 3)) + "\n")
        args = [MODS, G1, G6, "o1.png", "o2.png", "k1%s.npz" % tag, "k2%s.npz" % tag, "m%s.txt" % tag, "log%s.txt" % tag, "0", "1", "H.txt",
                config, os.path.join(CFG, "iters_one_view.ini")]
        p = subprocess.run(args, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.decode(), p.stderr.decode()

    out, err = run(str(tmp_path / "c.ini"), "a")
    lines = err.splitlines()
    at = lines.index("Overlap matches with E < 0.09")
    n_cli = int(lines[at + 1])
    assert lines[at + 2] == "" or lines[at + 2].startswith("HessianAffine: ")
    r1, r2 = _npz_regions(tmp_path / "k1a.npz"), _npz_regions(tmp_path / "k2a.npz")
    kw = dict(max_error=0.09, oriented=1, one_to_one=1, w1=800, h1=640, w2=800, h2=640)
    m, c = gpu_ctx.match_overlap(r1, r2, pkg.OverlapParams.default(H, **kw))
    assert n_cli == c.n_matches > 0
    assert "HessianAffine: %d | %d regions in the common area, repeatability " % (c.n_q_common, c.n_t_common) in err      # verbose = 1
    out0, err0 = run(os.path.join(CFG, "classic.ini"), "b")
    assert "verlap" not in err0 and "verlap" not in out0
    assert (tmp_path / "mb.txt").read_bytes() == (tmp_path / "ma.txt").read_bytes() and b"verlap" not in (tmp_path / "mb.txt").read_bytes()
    la, lb = (tmp_path / "loga.txt").read_text().split(), (tmp_path / "logb.txt").read_text().split()
    assert len(la) == len(lb) == 10 and la[1:] == lb[1:]              # (the first field is the run time)
    # without the ground truth there is nothing to match against: a note, no count
    p = subprocess.run([MODS, G1, G6, "o1.png", "o2.png", "k1c.npz", "k2c.npz", "mc.txt", "logc.txt", "1", "0", "Hc.txt", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and "doOverlapMatch needs the ground truth homography" in p.stderr.decode()
    assert "Overlap matches" not in p.stderr.decode()
