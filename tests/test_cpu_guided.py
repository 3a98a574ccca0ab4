"""CPU tests (no GPU) of guided matching: every refusal of mods_match_guided / mods_match_guided_reps comes with MODS_E_ARG and a
message before any device call, the command line rejects bad guided* keys while it parses the configuration, and the numpy
reference of the contract (tests/guided_ref.py) gives a hand-computed case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guided_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
EYE = (1, 0, 0, 0, 1, 0, 0, 0, 1)
NAN, INF = float("nan"), float("inf")


def _params(pkg, **kw):
    a = dict(model_type=0, model=EYE, radius=4.0, ratio=0.9, contradDist=10.0, max_dist=0, one_to_one=1)
    a.update(kw)
    return pkg.GuidedParams(a["model_type"], (C.c_double * 9)(*a["model"]), a["radius"], a["ratio"], a["contradDist"], a["max_dist"],
                            a["one_to_one"])


REFUSALS = [
    (dict(model_type=2), {}, b"model_type 2"), (dict(model_type=-1), {}, b"model_type -1"),
    (dict(model=(1, 0, 0, 0, NAN, 0, 0, 0, 1)), {}, b"model entry 4 is not finite"),
    (dict(model=(1, 0, 0, 0, 1, 0, 0, 0, INF), model_type=1), {}, b"model entry 8 is not finite"),
    (dict(model=(1, 2, 3, 2, 4, 6, 0, 0, 1)), {}, b"singular homography"),
    (dict(model=(0,) * 9), {}, b"singular homography"),
    (dict(radius=0.0), {}, b"radius 0"), (dict(radius=-1.0), {}, b"radius -1"), (dict(radius=INF), {}, b"radius inf"),
    (dict(radius=NAN), {}, b"radius"),
    (dict(ratio=0.0), {}, b"ratio 0 outside (0, 1]"), (dict(ratio=1.5), {}, b"ratio 1.5 outside (0, 1]"), (dict(ratio=NAN), {}, b"ratio"),
    (dict(contradDist=-0.5), {}, b"contradDist -0.5"), (dict(contradDist=INF), {}, b"contradDist inf"),
    (dict(max_dist=-1), {}, b"max_dist -1 < 0"),
    ({}, dict(n_q=-1), b"negative count"), ({}, dict(n_t=-7), b"negative count"),
    ({}, dict(q=None), b"null argument"), ({}, dict(t=None), b"null argument"), ({}, dict(par=None), b"null argument"),
    ({}, dict(n_out=None), b"null argument"), ({}, dict(out=None), b"null argument"),
    ({}, {}, b"null context"),
    (dict(model_type=1, model=(0,) * 9), {}, b"null context"),      # (a fundamental matrix is not inverted: no rank test)
    ({}, dict(q=None, n_q=0, t=None, n_t=0), b"null context")]      # (empty lists need no arrays)


@pytest.mark.parametrize("pkw,akw,msg", REFUSALS)
def test_match_guided_argument_errors(pkg, pkw, akw, msg):
    """mods_match_guided: MODS_E_ARG and a message, without a device and without a context"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, n_q=5, t=BUF, n_t=6, par=C.byref(par), out=BUF, n_out=BUF)
    a.update(akw)
    rc = lib.mods_match_guided(None, a["q"], a["n_q"], a["t"], a["n_t"], a["par"], a["out"], BUF, BUF, 8, a["n_out"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_guided: ") and msg in err, err


@pytest.mark.parametrize("pkw,akw,msg", [r for r in REFUSALS if not ({"n_q", "n_t"} & set(r[1]))])
def test_match_guided_reps_argument_errors(pkg, pkw, akw, msg):
    """mods_match_guided_reps: the same refusals; the banks are not looked at before the last of them"""
    lib = pkg.lib()
    par = _params(pkg, **pkw)
    a = dict(q=BUF, t=BUF, par=C.byref(par), out=BUF, n_out=BUF)
    a.update(akw)
    rc = lib.mods_match_guided_reps(None, a["q"], a["t"], a["par"], a["out"], BUF, BUF, 8, a["n_out"])
    assert rc == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_guided: ") and msg in err, err


def test_guided_params_layout_and_default(pkg):
    assert C.sizeof(pkg.GuidedParams) == 8 + 72 + 24 + 8          # int + pad, 9 doubles, 3 doubles, 2 ints
    p = pkg.GuidedParams.default(np.arange(9.0), model_type=1)
    assert list(p.model) == list(range(9)) and p.model_type == 1
    assert (p.radius, p.ratio, p.contradDist, p.max_dist, p.one_to_one) == (4.0, 0.9, 10.0, 0, 1)
    assert "guided" in pkg.STAGES and pkg.STAGES.index("guided") == 17


@pytest.mark.parametrize("key,value,msg", [("guidedRatio", "1.5", "guidedRatio must lie in (0, 1]"),
                                           ("guidedRadius", "0", "guidedRadius must be a positive"),
                                           ("guidedMaxDist", "-3", "guidedMaxDist must not be negative"),
                                           ("guidedMatching", "2", "guidedMatching must be 0 or 1")])
def test_cli_rejects_bad_guided_keys_at_parse_time(pkg, tmp_path, key, value, msg):
    """before the images are read and before any device call: neither image exists"""
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "[Matching]\n" in ini
    (tmp_path / "c.ini").write_text(ini.replace("[Matching]\n", "[Matching]\nguidedMatching = 1\n%s = %s\n" % (key, value))
                                    if key != "guidedMatching" else ini.replace("[Matching]\n", "[Matching]\nguidedMatching = 2\n"))
    p = subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and msg in err and "no_such_1.png" not in err, err


def test_cli_accepts_good_guided_keys(pkg, tmp_path):
    """a valid guided configuration gets past the parser (and then stops at the first missing image)"""
    ini = open(os.path.join(CFG, "classic.ini")).read()
    (tmp_path / "c.ini").write_text(ini.replace("[Matching]\n", "[Matching]\nguidedMatching = 1\nguidedRatio = 1\nguidedRadius = 2.5\n"))
    p = subprocess.run([MODS, "no_such_1.png", G6, "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and "no_such_1.png" in p.stderr.decode() and "guided" not in p.stderr.decode()


def _regions(xy, desc):
    r = np.zeros(len(xy), gr.REGION_DTYPE)
    r["x"], r["y"] = np.asarray(xy, np.float64).T
    r["s"] = 2.0 + np.arange(len(xy)); r["a11"] = 1.0; r["a22"] = 1.0; r["a12"] = 0.25; r["a21"] = -0.5
    r["desc"] = desc
    return r


def test_guided_ref_hand_computed_case():
    """3 queries x 3 trains under the translation by (3, 4), r = 5.
    Query 0 at (10, 10) is sent to (13, 14).  Train 0 at (16, 18): offset (3, 4), exactly on the radius - gated.  Train 1 at (13, 14):
    offset 0 - gated.  Train 2 at (13, 19.25): offset 5.25 - not gated.
    Query 1 at (100, 100) -> (103, 104): nothing within 5.  Query 2 at (7, 6) -> (10, 10): train 1 at distance 5 exactly ((3, 4) again).
    Descriptors: query 0 = all 10; trains 0 and 1 both all 12 (a tie at d = 128 * 4 = 512: the lower index, train 0, is t1);
    query 2 = all 13 (d to train 1 = 128).
    contradDist 4: train 1 lies 5 from train 0, so it is query 0's t_bad with d2 = 512; ratio test 512 < rho2 * 512 fails for every
    rho <= 1: query 0 is rejected.  contradDist 5: 25 > 25 is false, no t_bad: accepted with d2 = 0, ratio = 0."""
    H = (1, 0, 3, 0, 1, 4, 0, 0, 1)
    q = _regions([(10, 10), (100, 100), (7, 6)], np.array([[10] * 128, [50] * 128, [13] * 128], np.uint8))
    t = _regions([(16, 18), (13, 14), (13, 19.25)], np.array([[12] * 128, [12] * 128, [10] * 128], np.uint8))
    g = gr.gate_rows(0, H, 5.0, q, t, 0, 3)
    assert g.tolist() == [[True, True, False], [False, False, False], [False, True, False]]
    assert not gr.gate_rows(0, H, np.nextafter(5.0, 0.0), q, t, 0, 3)[0, 0]         # a hair inside the boundary: gone
    tent, u6, laf = gr.guided_ref(q, t, 0, H, 5.0, 1.0, 4.0)
    assert tent["q"].tolist() == [2] and tent["t"].tolist() == [1] and tent["t_bad"].tolist() == [-1]
    assert tent["d1"].tolist() == [128.0] and tent["d2"].tolist() == [0.0] and tent["ratio"].tolist() == [0.0]
    tent, u6, laf = gr.guided_ref(q, t, 0, H, 5.0, 1.0, 5.0)
    assert tent["q"].tolist() == [0, 2] and tent["t"].tolist() == [0, 1] and tent["t_bad"].tolist() == [-1, -1]
    assert tent["d1"].tolist() == [512.0, 128.0] and np.all(tent["t_2nd"] == -1) and np.all(tent["d2nd"] == 0)
    assert u6.tolist() == [[10, 10, 1, 16, 18, 1], [7, 6, 1, 13, 14, 1]]
    assert laf[0].tolist() == [10, 10, 1, 0.25, -0.5, 1, 2, 16, 18, 1, 0.25, -0.5, 1, 2]
    # max_dist exactly at d1 keeps, one below drops
    assert gr.guided_ref(q, t, 0, H, 5.0, 1.0, 5.0, max_dist=128)[0]["q"].tolist() == [2]
    assert gr.guided_ref(q, t, 0, H, 5.0, 1.0, 5.0, max_dist=127)[0]["q"].tolist() == []
    # an inconsistent second far enough in descriptor space: query 0 passes with its ratio
    t2 = t.copy(); t2["desc"][1] = 14                               # d(q0, t1) = 128 * 16 = 2048
    tent, _, _ = gr.guided_ref(q, t2, 0, H, 5.0, 0.6, 4.0)          # 512 < 0.36 * 2048 = 737.28
    assert tent["q"].tolist() == [0, 2] and tent["t_bad"].tolist() == [1, -1] and tent["d2"].tolist() == [2048.0, 0.0]
    assert tent["ratio"][0] == 0.5
    assert gr.guided_ref(q, t2, 0, H, 5.0, 0.5, 4.0)[0]["q"].tolist() == [2]      # 512 < 0.25 * 2048 = 512 is false
    # one to one: queries 0 and 2 both on train 1 once train 0 is gone; the smaller d1 stays, the other is not re-assigned
    t3 = t[1:].copy()
    tent, _, _ = gr.guided_ref(q, t3, 0, H, 5.0, 1.0, 5.0, one_to_one=0)
    assert tent["q"].tolist() == [0, 2] and tent["t"].tolist() == [0, 0]
    tent, _, _ = gr.guided_ref(q, t3, 0, H, 5.0, 1.0, 5.0, one_to_one=1)
    assert tent["q"].tolist() == [2] and tent["d1"].tolist() == [128.0]


def test_guided_ref_model_layouts():
    m = np.arange(9.0)
    assert gr.model_entries(0, m)[1][2] == 5.0 and gr.model_entries(1, m)[1][2] == 7.0      # F[3 * c + r] = entry (r, c)
    Hi = gr.invert3(gr.model_entries(0, (1, 0, 3, 0, 1, 4, 0, 0, 1)))
    assert Hi == [[1, 0, -3], [0, 1, -4], [0, 0, 1]]
    assert gr.invert3(gr.model_entries(0, (1, 2, 3, 2, 4, 6, 0, 0, 1))) is None
