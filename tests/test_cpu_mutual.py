"""The mutual check of the FGINN matcher (mods_ctx_match_mutual, csrc/mutual.hip) without a GPU: a worked case of the numpy
restatement (tests/mutual_ref.py), the refusals that need no device, and the command line's [Matching] mutualCheck."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mutual_ref as mr
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read


def _regions(xy, desc2):
    r = np.zeros(len(xy), orc.REGION_DTYPE)
    r["x"], r["y"] = np.asarray(xy, np.float64).T
    r["s"] = 2.0; r["a11"] = 1.0; r["a22"] = 1.0
    r["desc"][:, :2] = desc2
    return r


def _tent(pairs):
    t = np.zeros(len(pairs), orc.TENT_DTYPE)
    t["q"], t["t"] = np.asarray(pairs).T
    return t


def test_mutual_ref_hand_computed_case():
    """4 queries x 3 trains, descriptors zero but for their first two bytes.
    Trains: T0 = (10, 0), T1 = (10, 4), T2 = (200, 200).
    Queries 0, 1, 2 = (10, 0): three twins of T0 (d = 0), at (0, 0), (3, 4) - 5 from query 0, inside contradDist 10 - and (50, 0),
    outside it.  Query 3 = (10, 1) at (200, 0): d to T1 = 9; the twins lie at d = 16 from T1 and far from query 3.
    Forward tentatives: (0, T0), (1, T0), (2, T0), (3, T1).
    Mode 1: of the three at d = 0 the lowest index stays: query 0; query 3 is T1's nearest query.  Kept: 0 and 3.
    Mode 2, ratio 0.8 (ratio^2 = 0.64): query 0 has the far rival 2 at d_r = 0: 0 / 0 is NaN, which fails - dropped, as are 1 and 2.
      Query 3: every rival is far, quotient 9 / 16 = 0.5625 <= 0.64 - kept.
    Mode 2, ratio 0.7 (0.49): 0.5625 > 0.49 - query 3 is dropped too.
    Mode 2, contradDist 1e9: no rival is far, the ratio test never applies: mode 1's answer.
    Query 2 changed to (10, 200) (d = 40000 to T0, its tentative gone): query 0's only twin is query 1, inside contradDist, and the far
      rival passes with quotient 0 - query 0 is kept in mode 2; query 1 still loses the tie by index."""
    t = _regions([(5, 5), (60, 60), (300, 300)], [(10, 0), (10, 4), (200, 200)])
    q = _regions([(0, 0), (3, 4), (50, 0), (200, 0)], [(10, 0), (10, 0), (10, 0), (10, 1)])
    tent = _tent([(0, 0), (1, 0), (2, 0), (3, 1)])
    assert mr.sqdist(t["desc"][[1]], q["desc"]).tolist() == [[16, 16, 16, 9]]
    assert mr.keep_mask(tent, q, t, 0).tolist() == [True] * 4
    assert mr.keep_mask(tent, q, t, 1, 0.8, 10.0).tolist() == [True, False, False, True]
    assert mr.keep_mask(tent, q, t, 1, 0.7, 1.0).tolist() == [True, False, False, True]
    assert mr.keep_mask(tent, q, t, 2, 0.8, 10.0).tolist() == [False, False, False, True]
    assert mr.keep_mask(tent, q, t, 2, 0.7, 10.0).tolist() == [False, False, False, False]
    assert mr.keep_mask(tent, q, t, 2, 0.8, 1e9).tolist() == [True, False, False, True]
    q2 = q.copy()
    q2["desc"][2, :2] = (10, 200)
    tent2 = _tent([(0, 0), (1, 0), (3, 1)])
    assert mr.keep_mask(tent2, q2, t, 2, 0.8, 10.0).tolist() == [True, False, True]
    assert mr.keep_mask(tent2, q2, t, 2, 0.8, 4.0).tolist() == [False, False, True]      # contradDist 4: query 1 is now far, NaN again
    kept = mr.mutual_filter(tent, q, t, 1)
    assert kept["q"].tolist() == [0, 3] and kept["t"].tolist() == [0, 1]
    assert mr.u6_rows(kept, q, t).tolist() == [[0, 0, 1, 5, 5, 1], [200, 0, 1, 60, 60, 1]]
    assert mr.laf_rows(kept, q, t)[1].tolist() == [200, 0, 1, 0, 0, 1, 2, 60, 60, 1, 0, 0, 1, 2]
    assert len(mr.mutual_filter(tent[:0], q, t, 2)) == 0


@pytest.mark.parametrize("mode", [3, -1, 7])
def test_bad_modes_are_refused_without_a_device(pkg, mode):
    """mode outside 0 .. 2: MODS_E_ARG with a message, checked before the context or pipeline is looked at"""
    lib = pkg.lib()
    assert lib.mods_ctx_match_mutual(BUF, mode) == -2
    err = lib.mods_last_error()
    assert err.startswith(b"match_mutual: ") and ("mode %d" % mode).encode() in err, err
    assert lib.mods_pipeline_match_mutual(BUF, mode) == -2
    assert ("mode %d" % mode).encode() in lib.mods_last_error()


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    for mode in (0, 1, 2):
        assert lib.mods_ctx_match_mutual(None, mode) == -2 and b"null context" in lib.mods_last_error()
        assert lib.mods_pipeline_match_mutual(None, mode) == -2 and b"null pipeline" in lib.mods_last_error()
    n = C.c_int()
    assert lib.mods_match_mutual_counts(None, C.byref(n), C.byref(n)) == -2 and b"null argument" in lib.mods_last_error()
    assert lib.mods_match_mutual_counts(BUF, None, C.byref(n)) == -2 and b"null argument" in lib.mods_last_error()
    assert "match_mutual" in pkg.STAGES and pkg.STAGES.index("match_mutual") == 18


def _run_cli(tmp_path, line):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "[Matching]\n" in ini
    (tmp_path / "c.ini").write_text(ini.replace("[Matching]\n", "[Matching]\n" + line + "\n"))
    return subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                           os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("value", ["3", "-1"])
def test_cli_rejects_bad_mutual_check_at_parse_time(pkg, tmp_path, value):
    """before the images are read and before any device call: neither image exists"""
    p = _run_cli(tmp_path, "mutualCheck = " + value)
    err = p.stderr.decode()
    assert p.returncode == 1 and "mutualCheck must be 0, 1 or 2" in err and "no_such_1.png" not in err, err


@pytest.mark.parametrize("value", ["0", "1", "2"])
def test_cli_accepts_mutual_check(pkg, tmp_path, value):
    """a valid value gets past the parser (and the run then stops at the first missing image)"""
    p = _run_cli(tmp_path, "mutualCheck = " + value)
    err = p.stderr.decode()
    assert p.returncode == 1 and "no_such_1.png" in err and "mutualCheck" not in err, err
