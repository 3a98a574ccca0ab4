"""CPU tests (no GPU) of overlap matching: every refusal of mods_match_overlap / mods_match_overlap_reps comes with MODS_E_ARG and a
message before any device call, the command line rejects bad [OverlapMatching] keys while it parses the configuration, and the
numpy reference of the contract (tests/overlap_ref.py) gives a hand-computed case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import overlap_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G6 = os.path.join(ROOT, "tests", "golden", "graf6.png")
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
EYE = (1, 0, 0, 0, 1, 0, 0, 0, 1)
NAN, INF = float("nan"), float("inf")


def _params(pkg, **kw):
    a = dict(H=EYE, max_error=0.09, oriented=1, one_to_one=1, w1=0, h1=0, w2=0, h2=0)
    a.update(kw)
    return pkg.OverlapParams((C.c_double * 9)(*a["H"]), a["max_error"], a["oriented"], a["one_to_one"], a["w1"], a["h1"], a["w2"], a["h2"])


REFUSALS = [
    (dict(H=(1, 0, 0, 0, NAN, 0, 0, 0, 1)), {}, b"H entry 4 is not finite"),
    (dict(H=(1, 0, 0, 0, 1, 0, 0, 0, INF)), {}, b"H entry 8 is not finite"),
    (dict(H=(1, 2, 3, 2, 4, 6, 0, 0, 1)), {}, b"singular homography"),
    (dict(H=(0,) * 9), {}, b"singular homography"),
    (dict(H=(1e200, 0, 0, 0, 1e200, 0, 0, 0, 1)), {}, b"singular homography"),      # the determinant overflows
    (dict(max_error=0.0), {}, b"max_error 0"), (dict(max_error=-0.09), {}, b"max_error -0.09"), (dict(max_error=INF), {}, b"max_error inf"),
    (dict(max_error=NAN), {}, b"max_error"),
    (dict(oriented=2), {}, b"oriented 2"), (dict(oriented=-1), {}, b"oriented -1"),
    (dict(one_to_one=2), {}, b"one_to_one 2"), (dict(one_to_one=-1), {}, b"one_to_one -1"),
    (dict(w1=-1), {}, b"negative image size"), (dict(h1=-5), {}, b"negative image size"), (dict(w2=-1), {}, b"negative image size"),
    (dict(h2=-640), {}, b"negative image size"),
    ({}, dict(n_q=-1), b"negative count"), ({}, dict(n_t=-7), b"negative count"),
    ({}, dict(q=None), b"null argument"), ({}, dict(t=None), b"null argument"), ({}, dict(par=None), b"null argument"),
    ({}, dict(n_out=None), b"null argument"), ({}, dict(out=None), b"null argument"), ({}, dict(counts=None), b"null argument"),
    ({}, {}, b"null context"),
    (dict(w1=800, h1=640, w2=800, h2=640, oriented=0, one_to_one=0), {}, b"null context"),
    ({}, dict(q=None, n_q=0, t=None, n_t=0), b"null context"),      # (empty lists need no arrays)
    ({}, dict(out=None, max_out=0), b"null context")]               # (no room asked for: no array)


@pytest.mark.parametrize("pkw,akw,msg", REFUSALS)
def test_match_overlap_argument_errors(pkg, pkw, akw, msg):
    """mods_match_overlap: MODS_E_ARG and a message, without a device and without a context"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, n_q=5, t=BUF, n_t=6, par=C.byref(par), out=BUF, max_out=8, n_out=BUF, counts=BUF)
    a.update(akw)
    rc = lib.mods_match_overlap(None, a["q"], a["n_q"], a["t"], a["n_t"], a["par"], a["out"], a["max_out"], a["n_out"], a["counts"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_overlap: ") and msg in err, err


@pytest.mark.parametrize("pkw,akw,msg", [r for r in REFUSALS if not ({"n_q", "n_t"} & set(r[1]))])
def test_match_overlap_reps_argument_errors(pkg, pkw, akw, msg):
    """mods_match_overlap_reps: the same refusals; the banks are not looked at before the last of them"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, t=BUF, par=C.byref(par), out=BUF, max_out=8, n_out=BUF, counts=BUF)
    a.update(akw)
    rc = lib.mods_match_overlap_reps(None, a["q"], a["t"], a["par"], a["out"], a["max_out"], a["n_out"], a["counts"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_overlap: ") and msg in err, err


def test_overlap_splits_refusals(pkg):
    assert pkg.lib().mods_ctx_overlap_splits(None, 0) == -2 and pkg.lib().mods_ctx_overlap_splits(BUF, -1) == -2


def _grid_formula(search, n_q, n_t, forced):
    """the split plan as the three searches wrote it out before they shared it: ceil(n_q / 256) query blocks, as many splits of the
    256-train tiles as bring the grid to 2048 (guided) or 4096 (overlap, area-overlap) blocks unless the overlap knob forces a count,
    and the split count that the tiles per split leave.  (The guided search returned before this arithmetic when a list was empty;
    there the guards of the other two stand in.)"""
    qblocks, n_tiles = (n_q + 255) // 256, (n_t + 255) // 256
    splits = max(1, min(n_tiles, ((2048 if search == 0 else 4096) + qblocks - 1) // max(qblocks, 1)))
    if search == 1 and forced > 0:
        splits = max(1, min(n_tiles, forced))
    tiles_per_split = max(1, (n_tiles + splits - 1) // splits)
    return qblocks, max(1, (n_tiles + tiles_per_split - 1) // tiles_per_split), tiles_per_split


def test_list_search_grid(pkg):
    """mods_list_search_grid: the sweeps' split plan.  No result depends on it, the speed of the sweeps does
    (profiles/overlap_area_timing.txt: 7.0 ms with 1 split, 4.3 ms with 16), so the choice is pinned here"""
    GUIDED, OVERLAP = 0, 1
    for search, n_q, n_t, forced, want in [(OVERLAP, 5000, 4099, 0, (20, 17, 1)), (OVERLAP, 5000, 4099, 3, (20, 3, 6)),
                                           (OVERLAP, 60156, 47177, 0, (235, 17, 11)), (GUIDED, 60156, 47177, 0, (235, 9, 21)),
                                           (OVERLAP, 0, 5, 0, (0, 1, 1))]:
        assert pkg.list_search_grid(search, n_q, n_t, forced) == want == _grid_formula(search, n_q, n_t, forced)
    for search in (GUIDED, OVERLAP):
        for n_q in (0, 1, 256, 257, 5000, 60156):
            for n_t in (0, 1, 256, 257, 4099, 47177):
                for forced in (0, 1, 3, 1000):
                    got = pkg.list_search_grid(search, n_q, n_t, forced)
                    assert got == _grid_formula(search, n_q, n_t, forced), (search, n_q, n_t, forced)
                    # every train lies in a split and no split is empty
                    assert got[1] >= 1 and got[2] >= 1 and (got[1] - 1) * got[2] * 256 < max(n_t, 1) <= got[1] * got[2] * 256
    assert pkg.list_search_grid(GUIDED, 300, 257, 7) == pkg.list_search_grid(GUIDED, 300, 257)      # the guided search has no knob
    lib = pkg.lib()
    out = (C.c_int * 3)()
    for args in ((2, 5, 5, 0), (-1, 5, 5, 0), (1, -1, 5, 0), (1, 5, -1, 0), (1, 5, 5, -1)):
        assert lib.mods_list_search_grid(*args, out) == -2 and lib.mods_last_error().startswith(b"list_search_grid: ")
    assert lib.mods_list_search_grid(1, 5, 5, 0, None) == -2


def test_overlap_layouts_and_defaults(pkg):
    assert C.sizeof(pkg.OverlapParams) == 72 + 8 + 6 * 4           # 9 doubles, a double, 6 ints
    assert C.sizeof(pkg.OverlapCounts) == 16 + 8                   # 3 ints + pad, a double
    assert pkg.OVERLAP_DTYPE.itemsize == 32 and pkg.OVERLAP_DTYPE == orf.OVERLAP_DTYPE
    p = pkg.OverlapParams.default(np.arange(9.0))
    assert list(p.H) == list(range(9))
    assert (p.max_error, p.oriented, p.one_to_one, p.w1, p.h1, p.w2, p.h2) == (0.09, 1, 1, 0, 0, 0, 0)
    p = pkg.OverlapParams.default(None, max_error=0.2, oriented=0, one_to_one=0, w1=8, h1=6, w2=4, h2=2)
    assert list(p.H) == list(EYE) and (p.max_error, p.oriented, p.one_to_one, p.w1, p.h1, p.w2, p.h2) == (0.2, 0, 0, 8, 6, 4, 2)
    assert pkg.STAGES.index("overlap") == 19 and pkg.STAGES.index("guided") == 17 and pkg.STAGES.index("match_mutual") == 18


def _ini(tmp_path, body):
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "OverlapMatching" not in ini
    (tmp_path / "c.ini").write_text(ini + "\n[OverlapMatching]\n" + body)
    return str(tmp_path / "c.ini")


@pytest.mark.parametrize("body,msg", [("doOverlapMatch = 1\noverlapError = 0\n", "overlapError must be a positive number"),
                                      ("doOverlapMatch = 1\noverlapError = -0.09\n", "overlapError must be a positive number"),
                                      ("doOverlapMatch = 2\n", "doOverlapMatch must be 0 or 1"),
                                      ("doOverlapMatch = 1\nmatchOriented = 3\n", "matchOriented must be 0 or 1")])
def test_cli_rejects_bad_overlap_keys_at_parse_time(pkg, tmp_path, body, msg):
    """before the images are read and before any device call: neither image exists"""
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    p = subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", _ini(tmp_path, body),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and msg in err and "no_such_1.png" not in err, err


def test_cli_accepts_good_overlap_keys(pkg, tmp_path):
    """a valid configuration gets past the parser (and then stops at the first missing image)"""
    (tmp_path / "H.txt").write_text("1 0 0\n0 1 0\n0 0 1\n")
    p = subprocess.run([MODS, "no_such_1.png", G6, "o1", "o2", "k1", "k2", "m", "log", "0", "1", "H.txt",
                        _ini(tmp_path, "doOverlapMatch = 1\noverlapError = 0.2\nmatchOriented = 0\n"), os.path.join(CFG, "iters_one_view.ini")],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and "no_such_1.png" in p.stderr.decode() and "verlap" not in p.stderr.decode()


S4, S8 = 4.0 / 3.0, 8.0 / 3.0


def _regions(rows):
    """(x, y, s) rows with identity frames"""
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    return orf.regions(rows[:, :2], rows[:, 2], np.tile(np.eye(2), (len(rows), 1, 1)))


def test_overlap_ref_hand_computed_case():
    """H = the translation by (3, 4); identity frames; s = 4/3 gives 3 s = 4 exactly (s = 8/3: 8), so a query's C is 4 I, a train's I is
    I/4 (I/8), G = I (I/2), diff = 0 (0.5 (1/4 + 1/4) = 0.25) and dist = ((dx)^2 + (dy)^2) / 16 - every value below is exact.
      q0 (10, 10) -> (13, 14): t0 (14, 14) and t1 (13, 15) both at dist 1/16 = 0.0625 (a tie: t0), t2 (13, 14) with s = 8/3 at dist 0
        but diff 0.25 - with oriented = 0 the up-is-up form also takes the scale out (its determinant is 1), so there t2 has E = 0
        and is q0's choice.
      q1 (20, 10) -> (23, 14) and q2 (20, 10.75) -> (23, 14.75) both choose t3 (23, 14.5): E = 0.015625 and 0.00390625 - one to one
        keeps q2, q1 is dropped and not re-assigned.
      q3 (99, 50) -> (102, 54) lies outside a 100 x 100 image 2; its partner t4 (102, 54) comes back to (99, 50) and takes part.
      q4 (-3, 20) -> px == 0 exactly: excluded (0 < px is strict); its partner t5 (0, 24) comes back to bx = -3.
      q5 (0.5, 46) -> (3.5, 50) takes part; its partner t6 (3, 50) comes back to bx == 0 exactly: excluded."""
    assert 3.0 * S4 == 4.0 and 3.0 * S8 == 8.0
    H = (1, 0, 3, 0, 1, 4, 0, 0, 1)
    q = _regions([(10, 10, S4), (20, 10, S4), (20, 10.75, S4), (99, 50, S4), (-3, 20, S4), (0.5, 46, S4)])
    t = _regions([(14, 14, S4), (13, 15, S4), (13, 14, S8), (23, 14.5, S4), (102, 54, S4), (0, 24, S4), (3, 50, S4)])
    for oriented in (1, 0):
        E, dist, diff = orf.pair_errors(q, t, H, oriented)
        assert E.shape == (6, 7)
        e02, t_q0, e_q0 = (0.25, 0, 0.0625) if oriented else (0.0, 2, 0.0)
        assert E[0, :3].tolist() == [0.0625, 0.0625, e02] and dist[0, :3].tolist() == [0.0625, 0.0625, 0.0] and diff[0, :3].tolist() == [0, 0, e02]
        assert E[1, 3] == 0.015625 and E[2, 3] == 0.00390625 and E[3, 4] == 0 and E[4, 5] == 0 and E[5, 6] == 0.015625
        assert np.array_equal(orf.pair_errors(q, t, H, oriented, slice(1, 3))[0], E[1:3])
        assert np.array_equal(orf.pair_errors(q, t, H, oriented, np.array([5, 0]))[0], E[[5, 0]])
        # no image sizes: every region takes part
        m, c = orf.overlap_ref(q, t, orf.params(H, oriented=oriented, one_to_one=0))
        assert m["q"].tolist() == [0, 1, 2, 3, 4, 5] and m["t"].tolist() == [t_q0, 3, 3, 4, 5, 6]
        assert m["E"].tolist() == [e_q0, 0.015625, 0.00390625, 0, 0, 0.015625] and np.array_equal(m["E"], m["dist"]) and not m["diff"].any()
        assert (c.n_q_common, c.n_t_common, c.n_matches, c.repeatability) == (6, 7, 6, 1.0)
        m, c = orf.overlap_ref(q, t, orf.params(H, oriented=oriented, one_to_one=1))
        assert m["q"].tolist() == [0, 2, 3, 4, 5] and m["t"].tolist() == [t_q0, 3, 4, 5, 6] and c.repeatability == 5.0 / 6.0
        # the decision is strict: max_error at E itself rejects, the next double accepts
        tb = np.delete(t, 2)
        assert orf.overlap_ref(q, tb, orf.params(H, 0.0625, oriented, 0))[0]["q"].tolist() == [1, 2, 3, 4, 5]
        assert orf.overlap_ref(q, tb, orf.params(H, float(np.nextafter(0.0625, 1.0)), oriented, 0))[0]["q"].tolist() == [0, 1, 2, 3, 4, 5]
        # a wide bound does not change the choice: the smallest error, not the first below the bound
        m, _ = orf.overlap_ref(q[:1], t[[2, 1, 0]], orf.params(H, 0.3, oriented, 0))
        assert m["t"].tolist() == ([1] if oriented else [0]) and m["E"].tolist() == [e_q0]
        # the common area
        m, c = orf.overlap_ref(q, t, orf.params(H, oriented=oriented, one_to_one=0, w1=100, h1=100, w2=100, h2=100))
        assert m["q"].tolist() == [0, 1, 2] and m["t"].tolist() == [t_q0, 3, 3]
        assert (c.n_q_common, c.n_t_common, c.n_matches, c.repeatability) == (4, 5, 3, 0.75)
        m, c = orf.overlap_ref(q, t, orf.params(H, oriented=oriented, one_to_one=1, w1=100, h1=100, w2=100, h2=100))
        assert m["q"].tolist() == [0, 2] and (c.n_matches, c.repeatability) == (2, 0.5)
        mq, mt = orf.common_masks(q, t, orf.params(H, w1=100, h1=100, w2=100, h2=100))
        assert mq.tolist() == [True, True, True, False, False, True] and mt.tolist() == [True, True, True, True, True, False, False]
        # one size 0: no test at all
        assert orf.overlap_ref(q, t, orf.params(H, oriented=oriented, w1=100, h1=100, w2=100, h2=0))[1].n_q_common == 6
    # empty lists
    m, c = orf.overlap_ref(q, t[:0], orf.params(H, w1=100, h1=100, w2=100, h2=100))
    assert len(m) == 0 and (c.n_q_common, c.n_t_common, c.n_matches, c.repeatability) == (4, 0, 0, 0.0)


def test_overlap_ref_orientation_and_degenerates():
    """a frame rotated by 90 degrees is the same ellipse: rejected oriented (G is a rotation, diff = 2), accepted with up is up;
    singular frames and den == 0 give NaN, which is below nothing"""
    H = EYE
    R = np.array([[0.0, -1.0], [1.0, 0.0]])
    q = orf.regions([(50, 50)], [S4], [np.eye(2)])
    t = orf.regions([(50, 50)], [S4], [R])
    assert orf.pair_errors(q, t, H, 1)[0][0, 0] == 2.0 and orf.pair_errors(q, t, H, 0)[0][0, 0] == 0.0
    assert len(orf.overlap_ref(q, t, orf.params(H, oriented=1))[0]) == 0 and len(orf.overlap_ref(q, t, orf.params(H, oriented=0))[0]) == 1
    bad = orf.regions([(50, 50), (50, 50)], [S4, 0.0], [np.zeros((2, 2)), np.eye(2)])
    assert np.isnan(orf.pair_errors(q, bad, H, 1)[0]).all() and np.isnan(orf.pair_errors(q, bad, H, 0)[0]).all()
    Hs = (1, 0, 0, 0, 1, 0, 0.02, 0, -1.0)                         # den = 0.02 x - 1: zero on x = 50
    assert not np.isfinite(orf.pair_errors(q, t, Hs, 1)[0]).any()
    m, c = orf.overlap_ref(np.r_[q, q], np.r_[bad, t], orf.params(H, oriented=0))
    assert m["q"].tolist() == [0] and m["t"].tolist() == [2] and c.n_matches == 1
