"""ORSA-H a-contrario homography verification (useF = 3) on the host path (on_device=0, no device needed): the pieces against
their numpy restatement (tests/orsa_h_ref.py) to the bit, and whole calls on synthetic planar scenes.

There is no ORSA-H in the reference tree: the contract is the one in include/mods_hip.h (parity with the IPOL code unpinned).
The end-to-end bounds are the issue's: on scenes with inliers the result is significant, holds >= 90 % of the true inliers, is
>= 95 % true, and H transfers the noise-free points within 2 px; pure outliers give no model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import orsa_h_ref as ref  # noqa: E402

pkg = ge.load_package()
W, H = ref.W, ref.H
_runs = {}


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)   # as the hooks' out4 holds them


def scene_points(name):
    n, ratio, sigma, gseed, _ = ref.SCENES[name]
    return ref.scene(n, ratio, sigma, gseed)


def host_run(name):
    """the host path's result on a scene, computed once and shared (never modified)"""
    if name not in _runs:
        u6, _, _ = scene_points(name)
        _runs[name] = pkg.orsa_h(u6, None, W, H, seed_time=ref.SCENES[name][4], on_device=False)
    return _runs[name]


def random_samples(n, m, seed):
    rng = np.random.default_rng(seed)
    return np.array([np.sort(rng.choice(n, 4, replace=False)) for _ in range(m)], np.int32)


def check_against_ref(p1, p2, samples, out, Hs, tabs=None):
    tabs = tabs or ref.tables(len(p1))
    for j, s in enumerate(samples):
        c = np.concatenate([p1[s], p2[s]], 1)
        hm, valid = ref.solve_h4(c)
        assert np.array_equal(bits(hm), bits(Hs[j])), (j, hm, Hs[j])
        nfa, imin, la, bad, _ = ref.score(hm, valid, p1, p2, tabs)
        assert out[j, 3] == bad, j
        assert out[j, 0] == bits(nfa) and out[j, 1] == imin and out[j, 2] == bits(la), (j, nfa, imin, out[j])


@pytest.mark.parametrize("n,seed", [(5, 1), (9, 2), (60, 3)])
def test_solver_keys_nfa_equal_numpy(n, seed):
    u6, _, _ = ref.scene(n, 0.6, 1.0, 40 + seed)
    p1, p2, _ = ref.normalise(u6, W, H)
    samples = random_samples(n, 25, seed)
    out, Hs = pkg.orsa_h_test_score(p1, p2, W, H, samples, on_device=False)
    assert np.all(out[:, 3] == 0) and np.all(out[:, 0].view(np.float32) < 10000)
    check_against_ref(p1, p2, samples, out, Hs)


def test_tables_equal_numpy():
    for n in (5, 37, 200):
        a, b = pkg.orsa_h_test_tables(n)
        ra, rb = ref.tables(n)
        assert np.array_equal(bits(a), bits(ra)) and np.array_equal(bits(b), bits(rb))
        assert np.all(b[:5] == 0) and (n < 6 or b[6] == np.float32(np.log10(15.0)))


def _dyadic_points():
    """12 normalised points on a 1/8 grid, image 2 = image 1 shifted by (1/4, -1/8): every solve step is exact in fp64"""
    g = np.array([[0, 0], [2, 0], [4, 0], [2, 4], [-3, 1], [1, -2], [3, 3], [-1, -3], [-2, 2], [4, -1], [-4, -2], [0, 3]], np.float32) / 8
    return g.copy(), (g + np.array([0.25, -0.125], np.float32)).astype(np.float32)


def test_collinear_triple_and_duplicate_are_invalid():
    p1, p2 = _dyadic_points()
    p1[7], p2[7] = p1[4], p2[4]   # correspondence 7 duplicates 4: a zero pivot
    samples = np.array([[0, 1, 2, 3],    # 0, 1, 2 collinear (y = 0)
                        [3, 4, 5, 7],    # 4 and 7 identical
                        [3, 4, 5, 6]], np.int32)
    out, Hs = pkg.orsa_h_test_score(p1, p2, W, H, samples, on_device=False)
    assert list(out[:, 3]) == [1, 1, 0]
    for j in (0, 1):
        assert out[j, 0] == bits(np.float32(10000))[()] and out[j, 1] == 0 and np.all(Hs[j] == 0)
        assert not ref.solve_h4(np.concatenate([p1[samples[j]], p2[samples[j]]], 1))[1]
    check_against_ref(p1, p2, samples, out, Hs)


def test_exact_zero_error_is_clamped_to_flt_min():
    p1, _ = _dyadic_points()
    p1[3:7] = [[0, 0], [1, 0], [0, 1], [1, 1]]   # the sample: the unit square onto itself, a system of 0 and +-1 solved exactly
    p2 = p1.copy()
    p2[10:] = p2[10:] - np.float32(0.5)          # two correspondences off the identity
    samples = np.array([[3, 4, 5, 6]], np.int32)
    out, Hs = pkg.orsa_h_test_score(p1, p2, W, H, samples, on_device=False)
    assert np.array_equal(Hs[0], np.eye(3, dtype=np.float32).reshape(9))
    e = np.sort(ref.errors(Hs[0], p1, p2))
    assert np.all(e[:10] == 0) and e[10] > 0   # zero errors at sorted positions 4..9
    nfa = out[0, 0:1].view(np.float32)[0]
    la = out[0, 2:3].view(np.float32)[0]
    assert np.isfinite(nfa) and out[0, 1] == 9
    assert la == np.float32(np.float32(np.log10(np.pi)) + np.float32(np.log10(float(ref.FLT_MIN))))
    check_against_ref(p1, p2, samples, out, Hs)


def test_model_kind_helper():
    assert [pkg.model_kind(v) for v in (0, 1, 2, 3)] == [0, 1, 1, 0]
    for v in (-1, 4):
        with pytest.raises(pkg.ModsError):
            pkg.model_kind(v)


def test_argument_errors_and_small_lists():
    u6, _, _ = scene_points("n12_out")
    for w, h in ((0, H), (W, -1)):
        with pytest.raises(pkg.ModsError):
            pkg.orsa_h(u6, None, w, h, on_device=False)
    par = pkg.RansacParams.default(useF=3)
    u = np.ascontiguousarray(u6)
    mask, Hm, n = np.zeros(len(u), np.uint8), np.zeros(9), C.c_int()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L = pkg.lib()
    tail = (None, None, None, None, None, 0, 0, 0)
    E_ARG = L.mods_model_kind(-1)   # MODS_E_ARG
    assert E_ARG < 0
    assert L.mods_orsa_h_ex(vp(u), None, len(u), W, H, None, vp(mask), vp(Hm), C.byref(n), *tail) == E_ARG
    assert L.mods_orsa_h_ex(vp(u), None, len(u), W, H, C.byref(par), None, vp(Hm), C.byref(n), *tail) == E_ARG
    assert L.mods_orsa_h_ex(vp(u), None, len(u), W, H, C.byref(par), vp(mask), None, C.byref(n), *tail) == E_ARG
    assert L.mods_orsa_h_ex(vp(u), None, len(u), W, H, C.byref(par), vp(mask), vp(Hm), None, *tail) == E_ARG
    assert L.mods_orsa_h_ex(None, None, len(u), W, H, C.byref(par), vp(mask), vp(Hm), C.byref(n), *tail) == E_ARG
    for k in (0, 7):   # fewer than 8: no model, no error
        r = pkg.orsa_h(u6[:k], None, W, H, on_device=False)
        assert r["n"] == 0 and np.all(r["H"] == -1) and r["stats"] == [0, 0, 0] and r["log_nfa"] == 10000
    # the pair entry point refuses useF = 3 where it has no image size, as it refuses useF = 2
    pp = pkg.PairParams.default()
    pp.ransac = par
    tent = np.zeros(len(u6), pkg.TENT_DTYPE)
    with pytest.raises(pkg.ModsError, match="image size"):
        pkg.verify_tentatives(tent, u6, ref.laf_from_u6(u6), pp, seed_time=1)


@pytest.mark.parametrize("name", ref.SIGNIFICANT)
def test_scene_with_inliers(name):
    u6, inl, clean = scene_points(name)
    r = host_run(name)
    print(name, "log_nfa", r["log_nfa"], "subset", len(r["index"]), "true in subset", int(inl[r["index"]].sum()), "of", int(inl.sum()),
          "thr_px", r["thr_px"], "refit", r["refit"], "stats", r["stats"])
    assert r["log_nfa"] < -2
    sub = r["index"]
    assert len(sub) == r["n"] == r["mask"].sum() and np.array_equal(np.sort(sub), np.nonzero(r["mask"])[0])
    assert inl[sub].sum() >= 0.9 * inl.sum()
    assert inl[sub].sum() >= 0.95 * len(sub)
    d = np.linalg.norm(ref.apply_h(r["H"], clean[:, 0:2]) - clean[:, 2:4], axis=1)
    print(name, "largest transfer distance of the noise-free points", d.max())
    assert d.max() <= 2.0
    # thr_px is the largest error of the subset, in pixels: every member is within it, under H_out
    e = np.linalg.norm(ref.apply_h(r["H"], u6[sub, 0:2]) - u6[sub, 3:5], axis=1)
    assert e.max() <= r["thr_px"] * (1 + 1e-4) and e.max() >= r["thr_px"] * (1 - 1e-3)
    assert 1000 < r["stats"][0] <= 10000 and r["stats"][1] == r["stats"][0] + 1   # one model per iteration, and the refit


@pytest.mark.parametrize("name", ["n200_out", "n12_out"])
def test_pure_outliers_give_no_model(name):
    r = host_run(name)
    print(name, "log_nfa", r["log_nfa"])
    assert not r["log_nfa"] < -2
    assert np.all(r["H"] == -1) and r["n"] == 0 and not r["mask"].any() and r["thr_px"] == 0


def test_refit_taken_only_on_a_lower_nfa():
    seen = set()
    for name in ref.SCENES:
        loop, refit, taken = host_run(name)["refit"]
        assert taken == (1 if refit < loop else 0), (name, loop, refit, taken)
        assert bits(host_run(name)["log_nfa"]) == bits(min(loop, refit)), name
        seen.add(taken)
    # a least-squares fit of pure outliers does not beat the minimal model that set the record: both outcomes occur
    assert seen == {0, 1}, seen


def test_independent_of_batch_and_threads():
    name = "n200_r02"
    u6, _, _ = scene_points(name)
    want = host_run(name)
    for batch in (1, 77, 20000):
        r = pkg.orsa_h(u6, None, W, H, seed_time=ref.SCENES[name][4], on_device=False, batch=batch)
        for k in ("mask", "H", "index", "refit"):
            assert np.array_equal(r[k], want[k]), (batch, k)
        assert r["stats"][:2] == want["stats"][:2]   # (the third counts the rewinds, which are the blocking's own)
        assert (r["stats"][2] == 0) == (batch == 1)
        assert bits(r["log_nfa"]) == bits(want["log_nfa"]) and r["thr_px"] == want["thr_px"]
    code = ("import sys; sys.path.insert(0, %r); import test_cpu_orsa_h as c; import numpy as np; r = c.host_run(%r); "
            "np.save(sys.argv[1], np.concatenate([r['H'], r['index'], [float(r['log_nfa']), r['thr_px']], r['stats'][:2]]))"
            % (os.path.join(ROOT, "tests"), name))
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "orsa_h_threads_%d.npy" % os.getpid())
    out = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, MODS_RANSAC_THREADS="1"), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.load(path)
    os.remove(path)
    assert np.array_equal(got, np.concatenate([want["H"], want["index"], [float(want["log_nfa"]), want["thr_px"]], want["stats"][:2]]))


def _laf_error(Hm, laf):
    """sqrt of the summed HDsSymMax errors of the centre and the two frame points, per correspondence"""
    Hm = np.asarray(Hm).reshape(3, 3)
    Hi = np.linalg.inv(Hm)
    ks = 3.0
    tot = np.zeros(len(laf))
    for (ia, ib) in ((None, None), (3, 5), (2, 4)):
        a = laf[:, 0:2].copy()
        b = laf[:, 7:9].copy()
        if ia is not None:
            a += ks * laf[:, [ia, ib]] * laf[:, 6:7]
            b += ks * laf[:, [ia + 7, ib + 7]] * laf[:, 13:14]
        d1 = ((ref.apply_h(Hm, a) - b) ** 2).sum(1)
        d2 = ((ref.apply_h(Hi, b) - a) ** 2).sum(1)
        tot += np.maximum(d1, d2)
    return np.sqrt(tot)


def test_laf_check_runs_with_the_thr_px_bound():
    name = "n200_r05"
    u6, _, _ = scene_points(name)
    plain = host_run(name)
    laf = ref.laf_from_u6(u6)
    sub = np.sort(plain["index"])
    laf[sub[:6], 13] = 80.0   # six members of the subset get a frame in image 2 that the model cannot explain
    par = pkg.RansacParams.default(useF=3)
    r = pkg.orsa_h(u6, laf, W, H, params=par, seed_time=ref.SCENES[name][4], on_device=False)
    assert np.array_equal(r["H"], plain["H"]) and np.array_equal(r["index"], plain["index"]) and r["thr_px"] == plain["thr_px"]
    err = _laf_error(r["H"], laf)
    bound = par.HLAFCoef * r["thr_px"]
    assert not np.any(np.abs(err[sub] - bound) < 1e-6 * bound)
    want = sub[err[sub] <= bound]
    assert np.array_equal(np.nonzero(r["mask"])[0], want) and r["n"] == len(want) == len(sub) - 6
    # the bound follows thr_px: a coefficient under which even the consistent frames fail clears the list, H stays
    par.HLAFCoef = 0.9 * err[sub[6:]].min() / r["thr_px"]
    r2 = pkg.orsa_h(u6, laf, W, H, params=par, seed_time=ref.SCENES[name][4], on_device=False)
    assert r2["n"] == 0 and not r2["mask"].any() and np.array_equal(r2["H"], plain["H"])
    # and HLAFCoef = 0 switches the check off
    par.HLAFCoef = 0
    r3 = pkg.orsa_h(u6, laf, W, H, params=par, seed_time=ref.SCENES[name][4], on_device=False)
    assert np.array_equal(r3["mask"], plain["mask"])
