"""ORSA a-contrario F verification (useF = 2): the host pieces and the whole host path against recorded reference runs.

tests/golden/orsa_ref.npz was recorded from the reference's own orsa.cpp + libNumerics + libMatch, built outside this repository
with the reference's flags (g++ -O3 -ftree-vectorize -funroll-loops -ansi, Eigen 3.3.3 from its third_party tree), by a small
recorder that reads correspondences, calls srand(seed) and then orsa(w, h, match, index, 10000, verb 1, n_flag 1, mode 2, stop 0,
Fout) - n_flag 1 so that orsa() does not reseed - and writes the returned log(nfa), index, Fout and the iteration count it prints.
It also recorded 3000 epipolar() calls (F1, F2, z, root count) and makelogcombi_n / makelogcombi_k(7, .) tables.  Only the
recorded data is kept.  Inputs are synthetic two-view correspondences (_gen below); the largest case is stored as its generator
seed plus the sha256 of the float32 inputs.
"""
import hashlib
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
D = np.load(os.path.join(ROOT, "tests", "golden", "orsa_ref.npz"))
CASES = [str(c) for c in D["cases"]]
W, H = 800, 640


def _gen(n, ratio, seed, dup=0):
    """the recorder's generator: 3-D points seen by two cameras + uniform outliers, float32 n x 4 as Match (x1 y1 = image 2)"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1, 1, n), rng.uniform(4, 9, n)], 1)
    a = 0.08
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.6, 0.05, 0.1])
    f = 600.0

    def proj(P):
        return np.stack([f * P[:, 0] / P[:, 2] + W / 2, f * P[:, 1] / P[:, 2] + H / 2], 1)
    u1 = proj(X)
    u2 = proj(X @ R.T + t)
    u1 += rng.normal(0, 0.4, u1.shape)
    u2 += rng.normal(0, 0.4, u2.shape)
    nin = int(round(n * ratio))
    out = np.arange(nin, n)
    u2[out] = np.stack([rng.uniform(0, W, len(out)), rng.uniform(0, H, len(out))], 1)
    perm = rng.permutation(n)
    u1, u2 = u1[perm], u2[perm]
    m = np.concatenate([u2, u1], 1).astype(np.float32)
    if dup:
        src = rng.choice(n, dup, replace=False)
        dst = rng.choice(n, dup, replace=False)
        m[dst] = m[src]
    return m


def case_inputs(name):
    """(u6 in this project's layout: image 1 first, meta)"""
    meta = D[name + "_meta"]
    if name + "_match" in D:
        m = D[name + "_match"]
    else:
        m = _gen(int(meta[0]), float(D[name + "_ratio"]), int(meta[4]), int(meta[5]))
        assert hashlib.sha256(m.tobytes()).hexdigest().encode() == bytes(D[name + "_sha256"]), "regenerated inputs differ"
    ones = np.ones(len(m))
    u6 = np.stack([m[:, 2], m[:, 3], ones, m[:, 0], m[:, 1], ones], 1).astype(np.float64)
    return u6, meta


def check_run(name, r):
    meta = D[name + "_meta"]
    assert np.array([r["log_nfa"]], np.float32).view(np.uint32)[0] == D[name + "_nfa"][0], (name, r["log_nfa"])
    assert len(r["index"]) == meta[6]
    assert np.array_equal(r["index"], D[name + "_index"])
    assert r["stats"][0] == meta[7], (r["stats"], meta[7])
    Fref = D[name + "_F"].view(np.float64).reshape(3, 3)
    if r["log_nfa"] < -2:
        assert np.array_equal(r["F"].view(np.uint64), Fref.T.reshape(9).view(np.uint64))   # ransac_corresp.H = Fout^T
    else:
        assert np.all(r["F"] == -1) and r["n"] == 0 and not r["mask"].any()


def test_epipolar_bitwise():
    p1, p2, ks, ref = D["epi_p1"], D["epi_p2"], D["epi_k"], D["epi_out"]
    for c in range(len(ks)):
        F1, F2, z, m = pkg.orsa_test_epipolar(p1, p2, ks[c])
        want = ref[c]
        assert m == want[21], c
        assert np.array_equal(F1.view(np.uint32), want[:9]) and np.array_equal(F2.view(np.uint32), want[9:18]), c
        assert np.array_equal(z[:m].view(np.uint32), want[18:18 + m]), c


@pytest.mark.parametrize("n", [8, 20, 1000, 33000])
def test_logcombi_tables(n):
    a, b = pkg.orsa_test_tables(n)
    t = D["tab_%d" % n]
    assert np.array_equal(a.view(np.uint32), t[:n + 1]) and np.array_equal(b.view(np.uint32), t[n + 1:])


def test_log10_rounding():
    """glibc's (float)log10((double)x) through the host hook; the device equals it for every non-negative float (the sweep of
    tools/orsa_log10_sweep.py) - here a sample and the special values"""
    rng = np.random.default_rng(5)
    bits = np.concatenate([rng.integers(0, 0x7f800001, 200000, dtype=np.uint32),
                           np.array([0, 1, 0x7f800000, 0x3f800000, 0x41200000, 0x42c80000, 0x7f7fffff, 0x00800000], np.uint32)])
    x = bits.view(np.float32)
    got = pkg.orsa_test_log10(x)
    want = np.array([-np.inf if v == 0 else math.log10(v) for v in x.astype(np.float64).tolist()]).astype(np.float32)   # libm
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[-8] == -np.inf and got[-6] == np.inf and got[-5] == 0 and got[-4] == 1 and got[-3] == 2


@pytest.mark.parametrize("name", CASES)
def test_host_path_reproduces_reference(name):
    u6, meta = case_inputs(name)
    r = pkg.orsa_f(u6, None, int(meta[1]), int(meta[2]), seed_time=int(meta[3]), on_device=False)
    check_run(name, r)


def test_host_path_independent_of_batch():
    u6, meta = case_inputs("n300_r02")
    a = pkg.orsa_f(u6, None, W, H, seed_time=int(meta[3]), on_device=False, batch=7)
    b = pkg.orsa_f(u6, None, W, H, seed_time=int(meta[3]), on_device=False, batch=4000)
    check_run("n300_r02", a)
    check_run("n300_r02", b)
    assert a["stats"][:2] == b["stats"][:2]


def _laf_from_u6(u6, scale=3.0):
    n = len(u6)
    laf = np.zeros((n, 14))
    laf[:, 0:2] = u6[:, 0:2]
    laf[:, 7:9] = u6[:, 3:5]
    for o in (0, 7):
        laf[:, o + 2] = 1.0
        laf[:, o + 5] = 1.0
        laf[:, o + 6] = scale
    return laf


def test_filtering_wrapper_first_k_and_laf_check():
    """ORSAFiltering keeps the FIRST miniall + 1 tentatives in input order (matching.cpp:888-891), then F_LAF_check"""
    name = "n1000"
    u6, meta = case_inputs(name)
    k = int(meta[6]) + 1
    par = pkg.RansacParams.default(useF=2)
    par.LAFCoef = 0    # LAF check off
    r = pkg.orsa_f(u6, _laf_from_u6(u6), W, H, params=par, seed_time=int(meta[3]), on_device=False)
    check_run(name, r)
    assert r["n"] == k and np.array_equal(np.nonzero(r["mask"])[0], np.arange(k))
    # with the check, each error type keeps what F_LAF_check keeps of that prefix under its own error function
    laf = _laf_from_u6(u6)
    kept = {}
    for et in (0, 1, 2):
        par = pkg.RansacParams.default(useF=2)
        par.errorType = et
        r = pkg.orsa_f(u6, laf, W, H, params=par, seed_time=int(meta[3]), on_device=False)
        idx = np.nonzero(r["mask"])[0]
        assert r["n"] == len(idx) and np.array_equal(idx, _laf_expected(laf, r["F"], k, "FDs" if et == 0 else "FDsSym", 2.0 * 4.0))
        kept[et] = idx
    assert 8 <= len(kept[0]) < k and 8 <= len(kept[1]) < k            # the check removes some of the prefix, not all
    assert not np.array_equal(kept[0], kept[1])                        # Sampson (FDs) and symmetric (FDsSym) keep different sets
    assert np.array_equal(kept[1], kept[2])                            # SYMM_MAX and SYMM_SUM both use FDsSym


def _laf_expected(laf, F, k, fn, bound):
    """F_LAF_check (matching.cpp:192-249) of tentatives 0..k-1 written out, through the exported degensac error function"""
    import ctypes as C
    f = getattr(pkg.lib(), fn)
    Fc = np.ascontiguousarray(F, np.float64)
    keep = []
    for i in range(k):
        q = laf[i]
        ks = 3.0
        pts = [(q[0], q[1], q[7], q[8]),
               (q[0] + ks * q[3] * q[6], q[1] + ks * q[5] * q[6], q[7] + ks * q[10] * q[13], q[8] + ks * q[12] * q[13]),
               (q[0] + ks * q[2] * q[6], q[1] + ks * q[4] * q[6], q[7] + ks * q[9] * q[13], q[8] + ks * q[11] * q[13])]
        u = np.array([[a, b, 1.0, c, d, 1.0] for a, b, c, d in pts], np.float64)
        err = np.zeros(3)
        f(u.ctypes.data_as(C.c_void_p), Fc.ctypes.data_as(C.c_void_p), err.ctypes.data_as(C.c_void_p), 3)
        if not (np.sqrt(err[0]) + np.sqrt(err[1]) + np.sqrt(err[2]) > bound):
            keep.append(i)
    keep = np.array(keep, np.int64)
    return keep if len(keep) >= 8 else keep[:0]


def test_not_significant_and_small():
    u6, meta = case_inputs("n1000_r00")
    r = pkg.orsa_f(u6, None, W, H, seed_time=int(meta[3]), on_device=False)
    assert r["log_nfa"] > -2 and r["n"] == 0 and np.all(r["F"] == -1)
    u6s, _ = case_inputs("n20")
    r = pkg.orsa_f(u6s[:7], None, W, H, on_device=False)   # n < MIN_POINTS: nothing verified, no iteration
    assert r["n"] == 0 and r["stats"] == [0, 0, 0] and np.all(r["F"] == -1)


def test_argument_errors():
    u6, _ = case_inputs("n20")
    with pytest.raises(ValueError):
        pkg.orsa_f(u6[:, :5], None, W, H, on_device=False)
    with pytest.raises(pkg.ModsError):
        pkg.orsa_f(u6, None, 0, H, on_device=False)
    # the size-less verification entry point refuses useF = 2 instead of guessing an image size
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=2)
    tent = np.zeros(len(u6), pkg.TENT_DTYPE)
    with pytest.raises(pkg.ModsError, match="image size"):
        pkg.verify_tentatives(tent, u6, _laf_from_u6(u6), par)
