"""CPU tests (no GPU) of area-overlap matching: the numpy reference of the contract (tests/overlap_area_ref.py) gives the hand cases,
the assignment modes, the closed form of two circles and the gates; every refusal of mods_match_overlap_area[_reps] comes with
MODS_E_ARG and a message before any device call; the command line rejects bad overlapMeasure / overlapAreaError while it parses the
configuration."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import overlap_area_ref as oar
import overlap_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G6 = os.path.join(ROOT, "tests", "golden", "graf6.png")
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
EYE = (1, 0, 0, 0, 1, 0, 0, 0, 1)
NAN, INF = float("nan"), float("inf")
S10 = 10.0 / 3.0                # 3 s = 10 exactly: a circle of radius 10, 30 after the normalisation


def _circles(rows, s=S10):
    """(x, y) rows with identity frames"""
    rows = np.asarray(rows, np.float64).reshape(-1, 2)
    return orf.regions(rows, np.full(len(rows), s), np.tile(np.eye(2), (len(rows), 1, 1)))


def _counts(pairs):
    return [tuple(int(v) for v in (r["n_q_px"], r["n_t_px"], r["n_both"])) for r in pairs]


def test_hand_cases():
    """H = I, circles of radius 10: the lattice counts of the contract.  2821 is the number of lattice points of a disc of radius 30"""
    assert 3.0 * S10 == 10.0
    q = _circles([(100, 100), (101.2, 100)])
    t = _circles([(100, 100), (101, 100), (103, 100)])
    pairs = oar.evaluated_pairs(q, t, oar.params(EYE, max_error=0.4, one_to_one=0))
    assert [(int(r["q"]), int(r["t"])) for r in pairs] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    c = _counts(pairs)
    assert c[0] == (2821, 2821, 2821) and pairs["E"][0] == 0.0 and not np.signbit(pairs["E"][0])
    assert c[1] == (2821, 2821, 2642) and c[2] == (2821, 2821, 2288)
    assert c[4] == (2818, 2821, 2784) and c[5] == (2818, 2821, 2499)
    for r in pairs:
        uni = int(r["n_q_px"]) + int(r["n_t_px"]) - int(r["n_both"])
        assert r["E"] == 1.0 - float(r["n_both"]) / float(uni)
    # concentric circles, the train of 0.7 times the query's area
    t7 = orf.regions([(100, 100)], [S10], [np.eye(2) * np.sqrt(0.7)])
    assert _counts(oar.evaluated_pairs(q[:1], t7, oar.params(EYE, max_error=0.4))) == [(2821, 1993, 1993)]


def test_assignment_modes():
    q = _circles([(100, 100), (101.2, 100)])
    t = _circles([(101, 100), (103, 100)])
    pairs = oar.evaluated_pairs(q, t, oar.params(EYE, max_error=0.4))
    assert len(pairs) == 4 and (pairs["E"] < 0.4).all()
    m, c = oar.overlap_area_ref(q, t, oar.params(EYE, 0.4, 0), pairs)
    assert list(zip(m["q"].tolist(), m["t"].tolist())) == [(0, 0), (1, 0)] and (c.n_matches, c.repeatability) == (2, 1.0)
    m, c = oar.overlap_area_ref(q, t, oar.params(EYE, 0.4, 1), pairs)
    assert list(zip(m["q"].tolist(), m["t"].tolist())) == [(1, 0)] and (c.n_matches, c.repeatability) == (1, 0.5)
    m, c = oar.overlap_area_ref(q, t, oar.params(EYE, 0.4, 2), pairs)
    assert list(zip(m["q"].tolist(), m["t"].tolist())) == [(0, 1), (1, 0)] and c.n_matches == 2
    assert _counts(m) == [(2821, 2821, 2288), (2818, 2821, 2784)]
    # the decision is strict: max_error at E itself rejects, the next double accepts
    e = float(pairs["E"][1])                                          # (q0, t1)
    assert len(oar.assign(pairs[1:2], e, 0)) == 0 and len(oar.assign(pairs[1:2], float(np.nextafter(e, 1.0)), 0)) == 1
    # two identical trains: the lower index, in every mode
    t2 = _circles([(101, 100), (101, 100)])
    for mode in (0, 1, 2):
        m, _ = oar.overlap_area_ref(q[:1], t2, oar.params(EYE, 0.4, mode))
        assert m["t"].tolist() == [0]


def test_lattice_against_closed_form():
    """equal circles at 200 random offsets: the lattice count is within 0.01 of the closed form of two circles (the contract's
    prototype measured 0.0032)"""
    rng = np.random.default_rng(17)
    off = rng.uniform(-12.0, 12.0, (200, 2))
    q = _circles([(100, 100)])
    t = _circles(np.array([100.0, 100.0]) + off)
    pairs = oar.evaluated_pairs(q, t, oar.params(EYE, max_error=1.0))
    assert len(pairs) == 200
    want = np.array([oar.circle_overlap_error(30.0, 3.0 * float(np.hypot(*o))) for o in off])
    err = np.abs(pairs["E"] - want)
    print("largest |E - closed form| over 200 offsets: %.5f" % err.max())
    assert err.max() <= 0.01


def _frame_pair(A, tA=None, txy=(100, 100), ts=S10, **kw):
    q = orf.regions([(100, 100)], [S10], [A])
    t = orf.regions([txy], [ts], [A if tA is None else tA])
    return oar.evaluated_pairs(q, t, oar.params(EYE, **kw))


def test_gates():
    # the cap: a normalised half-length of 240 is walked, one of 270 is not
    p = _frame_pair(np.diag([8.0, 1.0 / 8.0]))
    assert len(p) == 1 and p["E"][0] == 0.0 and p["n_q_px"][0] == p["n_t_px"][0] == p["n_both"][0] > 2000
    assert len(_frame_pair(np.diag([9.0, 1.0 / 9.0]))) == 0
    assert len(_frame_pair(np.diag([1.0 / 9.0, 9.0]))) == 0
    # the area gate: g = 0.9 (1 - 0.4) = 0.54 either way
    for ratio, ev in ((0.5, 0), (0.53, 0), (0.55, 1), (1.0, 1), (1.8, 1), (1.9, 0), (2.0, 0)):
        assert len(_frame_pair(np.eye(2), np.eye(2) * np.sqrt(ratio))) == ev, ratio
    # ... and it follows max_error: with 0.5 the gate is 0.45
    assert len(_frame_pair(np.eye(2), np.eye(2) * np.sqrt(0.5), max_error=0.5)) == 1
    # what the gate removes is never below the bound: 1 - ratio >= max_error for concentric circles
    assert _frame_pair(np.eye(2), np.eye(2) * np.sqrt(0.55))["E"][0] > 0.4
    # disjoint boxes: 20 pixels apart the two boxes touch (|dx| == qex + tex is evaluated), beyond they do not
    assert len(_frame_pair(np.eye(2), txy=(120, 100))) == 1 and len(_frame_pair(np.eye(2), txy=(120.01, 100))) == 0
    assert len(_frame_pair(np.eye(2), txy=(100, 79.9))) == 0 and len(_frame_pair(np.eye(2), txy=(130, 130))) == 0
    p = _frame_pair(np.eye(2), txy=(120, 100))
    assert (int(p["n_q_px"][0]), int(p["n_t_px"][0]), int(p["n_both"][0])) == (2821, 2821, 1) and len(oar.assign(p, 0.4, 2)) == 0


def test_degenerate_inputs_never_match():
    """a singular frame, den == 0, NaN and inf: no evaluated pair, no exception"""
    q = _circles([(100, 100)])
    good = _circles([(101, 100)])
    bad = orf.regions([(100, 100)] * 6, [S10, 0.0, S10, S10, INF, -INF],
                      [np.zeros((2, 2)), np.eye(2), np.array([[1.0, 2.0], [2.0, 4.0]]), np.full((2, 2), NAN), np.eye(2), np.eye(2)])
    bad = np.r_[bad, orf.regions([(NAN, 100), (100, INF)], [S10, S10], [np.eye(2)] * 2)]
    with np.errstate(all="raise"):                                     # (the reference silences what it expects itself)
        for mode in (0, 1, 2):
            p = oar.params(EYE, 0.4, mode)
            assert len(oar.evaluated_pairs(q, bad, p)) == 0 and len(oar.evaluated_pairs(bad, q, p)) == 0
            assert len(oar.evaluated_pairs(bad, bad, p)) == 0
            m, c = oar.overlap_area_ref(np.r_[bad, q], np.r_[bad, good], p)
            assert m["q"].tolist() == [len(bad)] and m["t"].tolist() == [len(bad)] and c.n_matches == 1
        Hs = (1, 0, 0, 0, 1, 0, 0.01, 0, -1.0)                         # den = 0.01 x - 1: zero on x = 100
        assert len(oar.evaluated_pairs(q, good, oar.params(Hs))) == 0
        # max_error = 1 opens the area gate (g = 0): a train of no area is walked and counts nothing
        p = oar.evaluated_pairs(q, bad, oar.params(EYE, 1.0, 0))
        assert len(oar.assign(p, 1.0, 0)) == 0


# ---- the library without a device ------------------------------------------------------------------------------------------------

def _params(pkg, **kw):
    a = dict(H=EYE, max_error=0.4, one_to_one=2, w1=0, h1=0, w2=0, h2=0)
    a.update(kw)
    return pkg.OverlapAreaParams((C.c_double * 9)(*a["H"]), a["max_error"], a["one_to_one"], a["w1"], a["h1"], a["w2"], a["h2"])


REFUSALS = [
    (dict(H=(1, 0, 0, 0, NAN, 0, 0, 0, 1)), {}, b"H entry 4 is not finite"),
    (dict(H=(1, 0, 0, 0, 1, 0, 0, 0, INF)), {}, b"H entry 8 is not finite"),
    (dict(H=(1, 2, 3, 2, 4, 6, 0, 0, 1)), {}, b"singular homography"),
    (dict(H=(0,) * 9), {}, b"singular homography"),
    (dict(H=(1e200, 0, 0, 0, 1e200, 0, 0, 0, 1)), {}, b"singular homography"),      # the determinant overflows
    (dict(max_error=0.0), {}, b"max_error 0"), (dict(max_error=-0.4), {}, b"max_error -0.4"), (dict(max_error=INF), {}, b"max_error inf"),
    (dict(max_error=NAN), {}, b"max_error"), (dict(max_error=1.5), {}, b"max_error 1.5"),
    (dict(max_error=float(np.nextafter(1.0, 2.0))), {}, b"max_error 1"),
    (dict(one_to_one=3), {}, b"one_to_one 3"), (dict(one_to_one=-1), {}, b"one_to_one -1"),
    (dict(w1=-1), {}, b"negative image size"), (dict(h1=-5), {}, b"negative image size"), (dict(w2=-1), {}, b"negative image size"),
    (dict(h2=-640), {}, b"negative image size"),
    ({}, dict(n_q=-1), b"negative count"), ({}, dict(n_t=-7), b"negative count"),
    ({}, dict(q=None), b"null argument"), ({}, dict(t=None), b"null argument"), ({}, dict(par=None), b"null argument"),
    ({}, dict(n_out=None), b"null argument"), ({}, dict(out=None), b"null argument"), ({}, dict(counts=None), b"null argument"),
    ({}, {}, b"null context"),
    (dict(max_error=1.0, one_to_one=0), {}, b"null context"), (dict(one_to_one=1, w1=800, h1=640, w2=800, h2=640), {}, b"null context"),
    ({}, dict(q=None, n_q=0, t=None, n_t=0), b"null context"),      # (empty lists need no arrays)
    ({}, dict(out=None, max_out=0), b"null context")]               # (no room asked for: no array)


@pytest.mark.parametrize("pkw,akw,msg", REFUSALS)
def test_match_overlap_area_argument_errors(pkg, pkw, akw, msg):
    """mods_match_overlap_area: MODS_E_ARG and a message, without a device and without a context"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, n_q=5, t=BUF, n_t=6, par=C.byref(par), out=BUF, max_out=8, n_out=BUF, counts=BUF)
    a.update(akw)
    rc = lib.mods_match_overlap_area(None, a["q"], a["n_q"], a["t"], a["n_t"], a["par"], a["out"], a["max_out"], a["n_out"], a["counts"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_overlap_area: ") and msg in err, err


@pytest.mark.parametrize("pkw,akw,msg", [r for r in REFUSALS if not ({"n_q", "n_t"} & set(r[1]))])
def test_match_overlap_area_reps_argument_errors(pkg, pkw, akw, msg):
    """mods_match_overlap_area_reps: the same refusals; the banks are not looked at before the last of them"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, t=BUF, par=C.byref(par), out=BUF, max_out=8, n_out=BUF, counts=BUF)
    a.update(akw)
    rc = lib.mods_match_overlap_area_reps(None, a["q"], a["t"], a["par"], a["out"], a["max_out"], a["n_out"], a["counts"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_overlap_area: ") and msg in err, err


def test_overlap_area_layouts_and_defaults(pkg):
    assert C.sizeof(pkg.OverlapAreaParams) == 72 + 8 + 5 * 4 + 4           # 9 doubles, a double, 5 ints, padding
    assert pkg.OVERLAP_AREA_DTYPE.itemsize == 32 and pkg.OVERLAP_AREA_DTYPE == oar.AREA_DTYPE
    p = pkg.OverlapAreaParams.default(np.arange(9.0))
    assert list(p.H) == list(range(9))
    assert (p.max_error, p.one_to_one, p.w1, p.h1, p.w2, p.h2) == (0.4, 2, 0, 0, 0, 0)
    p = pkg.OverlapAreaParams.default(None, max_error=0.2, one_to_one=0, w1=8, h1=6, w2=4, h2=2)
    assert list(p.H) == list(EYE) and (p.max_error, p.one_to_one, p.w1, p.h1, p.w2, p.h2) == (0.2, 0, 8, 6, 4, 2)
    assert pkg.STAGES.index("overlap_area") == 20 == len(pkg.STAGES) - 1 and pkg.STAGES.index("overlap") == 19


def _ini(tmp_path, body):
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "OverlapMatching" not in ini
    (tmp_path / "c.ini").write_text(ini + "\n[OverlapMatching]\n" + body)
    return str(tmp_path / "c.ini")


@pytest.mark.parametrize("body,msg", [("doOverlapMatch = 1\noverlapMeasure = foo\n", "overlapMeasure must be linear or area"),
                                      ("overlapMeasure = Area\n", "overlapMeasure must be linear or area"),
                                      ("doOverlapMatch = 1\noverlapMeasure = area\noverlapAreaError = 0\n", "overlapAreaError must lie in (0, 1]"),
                                      ("doOverlapMatch = 1\noverlapMeasure = area\noverlapAreaError = 1.5\n", "overlapAreaError must lie in (0, 1]"),
                                      ("overlapAreaError = -0.4\n", "overlapAreaError must lie in (0, 1]")])
def test_cli_rejects_bad_area_keys_at_parse_time(pkg, tmp_path, body, msg):
    """before the images are read and before any device call: neither image exists"""
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    p = subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", _ini(tmp_path, body),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and msg in err and "no_such_1.png" not in err, err


@pytest.mark.parametrize("body", ["doOverlapMatch = 1\noverlapMeasure = area\noverlapAreaError = 0.5\n",
                                  "doOverlapMatch = 1\noverlapMeasure = area\noverlapAreaError = 1\n",
                                  "doOverlapMatch = 1\noverlapMeasure = linear\noverlapError = 0.2\n"])
def test_cli_accepts_good_area_keys(pkg, tmp_path, body):
    """a valid configuration gets past the parser (and then stops at the first missing image)"""
    (tmp_path / "H.txt").write_text("1 0 0\n0 1 0\n0 0 1\n")
    p = subprocess.run([MODS, "no_such_1.png", G6, "o1", "o2", "k1", "k2", "m", "log", "0", "1", "H.txt", _ini(tmp_path, body),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and "no_such_1.png" in p.stderr.decode() and "verlap" not in p.stderr.decode()
