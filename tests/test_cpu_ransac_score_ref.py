"""Anchors tests/ransac_score_ref.py - the numpy restatement that test_gpu_ransac_score.py judges the scoring and counting kernels
by - before it judges anything: to the bit against the library's host error functions, and against the reference's own
degensac build (oracle/_ref) where that exists.  The conditions the GPU test relies on (which models are degenerate, which
threshold bands are occupied, equality and exact zeros) are asserted here, on the reference alone.  No device."""
import ctypes as C

import numpy as np
import pytest

import ransac_score_cases as cases
import ransac_score_ref as ref
import refdeg


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    """equal to the bit where finite, equal NaN and infinity masks (NaN payloads are not compared)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
            and np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
            and np.array_equal(bits(got[fin]), bits(want[fin])))


def records_of(pkg, models):
    """(h, Hinv, H1) of every model as a scored record carries them (the library's sym_prepare; H1 = minv(Hinv) is an input of the
    restatement, not a part of it)"""
    ops = [pkg.host_sym_prepare(h) for h in models]
    return np.array(models), np.array([o[0] for o in ops]), np.array([o[1] for o in ops])


CPU_SHAPES = [(1, 1), (1, 17), (5, 8), (63, 16), (129, 17), (385, 130), (1000, 17)]


@pytest.mark.parametrize("ln,n", CPU_SHAPES)
def test_homography_errors_bitexact(pkg, ln, n):
    """HDs, HDsSym, HDsSymMax restated = the library's host functions = the reference's own, degenerate models included"""
    M = pkg.lib()
    u = cases.h_corr(ln, 7 + ln)
    models, degenerate = cases.h_models(u, n, ln)
    rec = records_of(pkg, models)
    if refdeg.available():
        R = refdeg.lib()
        Z = np.zeros(18 * ln)
        R.lin_hg(P(u), P(Z), P(np.arange(ln, dtype=np.int32)), ln)
    for k in range(n):
        h = np.ascontiguousarray(models[k])
        assert np.array_equal(bits(rec[1][k]), bits(ref.hinv_of(h)))
        for etype in (0, 1, 2):
            got, _ = ref.h_error(u, h, rec[1][k], rec[2][k], etype)
            want = np.zeros(ln)
            assert M.mods_test_host_errfn(etype, P(u), ln, P(h), 0, P(want)) == 0
            assert same(got, want), (k, etype, "library")
            for lanes in (1, 4, 8):                  # the LO step's vector forms carry NaN and infinity the same way
                v = np.zeros(ln)
                if M.mods_test_host_errfn(etype, P(u), ln, P(h), lanes, P(v)) == 0:
                    assert same(v, want), (k, etype, lanes)
            if refdeg.available():
                r = np.zeros(ln)
                getattr(R, ("HDs", "HDsSym", "HDsSymMax")[etype])(P(Z), P(u), P(h), P(r), ln)
                assert same(got, r), (k, etype, "reference")


@pytest.mark.parametrize("ln,n", [(1, 1), (1, 17), (63, 16), (129, 24), (385, 65), (1000, 17)])
def test_epipolar_errors_bitexact(pkg, ln, n):
    """FDs, FDsSym restated = the library's host functions = the reference's own"""
    M = pkg.lib()
    u, F = cases.f_corr(ln, 5 + ln)
    models, _ = cases.f_models(F, n, ln)
    for k in range(n):
        f = np.ascontiguousarray(models[k])
        for mode in (0, 1):
            got = ref.fds_sym(u, f) if mode else ref.fds(u, f)
            want, w = np.zeros(ln), np.zeros(ln)
            assert M.mods_test_host_fds(mode, P(u), ln, P(f), 0, P(want), P(w)) == 0
            assert same(got, want), (k, mode, "library")
            if refdeg.available():
                r = np.zeros(ln)
                getattr(refdeg.lib(), ("FDs", "FDsSym")[mode])(P(u), P(f), P(r), ln)
                assert same(got, r), (k, mode, "reference")


@pytest.mark.parametrize("ln", [1, 129, 385, 1000])
@pytest.mark.parametrize("th", [0.0, 16.0, "equal"])
def test_scores_against_inlidxs(pkg, ln, th):
    """J (the sequential sum of truncQuad) and I of the restatement = inlidxs of the library's host code and of the reference"""
    M = pkg.lib()
    u = cases.h_corr(ln, 7 + ln)
    models, degenerate = cases.h_models(u, 8, ln)
    d, s = ref.errors_h(u, records_of(pkg, models), 0)
    th = float(d[0, min(2, ln - 1)]) if th == "equal" else th
    want = ref.scores(d, s, 1, th, 9 * th)
    for k in range(len(models)):
        row = np.ascontiguousarray(d[k])
        if k not in degenerate:
            row[ln // 2] = th * 9 / 4           # the boundary of the truncation, met with equality
            want_k = ref.scores(row[None], s[k][None], 1, th, 9 * th)
        else:
            want_k = dict(J=want["J"][k:k + 1], I=want["I"][k:k + 1])
        inl, I, J = np.zeros(ln, np.int32), C.c_uint(), C.c_double()
        assert M.mods_test_host_inlidxs(P(row), ln, C.c_double(th), 0, P(inl), C.byref(I), C.byref(J)) == 0
        assert I.value == want_k["I"][0] and same(np.array([J.value]), want_k["J"]), k
        if refdeg.available():
            R = refdeg.lib()
            R.inlidxs.restype = refdeg.Score
            S = R.inlidxs(P(row), ln, C.c_double(th), P(inl))
            assert S.I == want_k["I"][0] and same(np.array([S.J]), want_k["J"]), k


def check_round(kind, ln, n, d, s, degenerate, rnd, want, exact_zero_model):
    """the conditions of one round, on the reference alone"""
    etype, do_sym, th_kind, th = rnd
    for k in range(n):
        finite = np.isfinite(d[k]).all() and np.isfinite(s[k]).all()
        # a degenerate model is non-finite in its error or in the symmetric check's operand (a horizon model leaves HDs finite)
        assert finite == (k not in degenerate), (kind, ln, n, k, etype)
    ok = [k for k in range(n) if k not in degenerate]
    vals = d[ok].ravel()
    if th_kind in ("fixed", "equal") and ln >= cases.PLANTED:
        assert np.any(vals <= th) and np.any((vals > th) & (vals < th * 9 / 4)) and np.any(vals >= th * 9 / 4), (kind, ln, n, rnd)
    if th_kind == "equal":
        assert th > 0 and d[0, min(2, ln - 1)] == th and want["I"][0] >= 1
    if th_kind == "zero":
        assert not np.any(want["J"]) and np.array_equal(want["I"], np.count_nonzero(d == 0, axis=1))
        if exact_zero_model is not None:
            assert want["I"][exact_zero_model] >= 1
    if th_kind == "huge":
        assert float(th) * 9 / 4 == float("inf")
        if n >= 3:
            assert np.isposinf(d).any()              # truncQuad's epsilon >= thr 9/4 is met with equality: gain 0, not NaN
        assert np.array_equal(want["J"][ok], np.full(len(ok), float(ln))) and np.array_equal(want["I"][ok], np.full(len(ok), ln))
    if not do_sym:
        assert not np.any(want["Isym"])
    elif th_kind != "zero" and ln >= cases.PLANTED:
        assert np.any(want["Isym"][ok] > 0)


@pytest.mark.parametrize("ln,n", cases.shapes(cases.H_NS))
def test_conditions_of_the_homography_rounds(pkg, ln, n):
    u = cases.h_corr(ln, 7 + ln)
    models, degenerate = cases.h_models(u, n, ln)
    rec = records_of(pkg, models)
    errs = {e: ref.errors_h(u, rec, e) for e in (0, 1, 2)}
    for etype, do_sym, th_kind in cases.rounds(ln, n, (0, 1, 2)):
        d, s = errs[etype]
        th = cases.round_th(th_kind, d, ln)
        want = ref.scores(d, s, do_sym, th, cases.H_CHECK_COEF * th)
        check_round("H", ln, n, d, s, degenerate, (etype, do_sym, th_kind, th), want, 2 if n >= 5 else None)


@pytest.mark.parametrize("ln,n", cases.shapes(cases.F_NS))
def test_conditions_of_the_epipolar_rounds(pkg, ln, n):
    u, F = cases.f_corr(ln, 5 + ln)
    models, degenerate = cases.f_models(F, n, ln)
    errs = {e: ref.errors_f(u, models, e) for e in (0, 1)}
    for etype, do_sym, th_kind in cases.rounds(ln, n, (0, 1)):
        d, s = errs[etype]
        th = cases.round_th(th_kind, d, ln)
        want = ref.scores(d, s, do_sym, th, cases.F_CHECK_COEF * th)
        check_round("F", ln, n, d, s, degenerate, (etype, do_sym, th_kind, th), want, 2 if n >= 4 else None)


def test_true_f_fits_the_scene():
    """cases.true_f is the matrix of fsynth.two_view's camera pair: the scene's inliers lie on it"""
    import fsynth
    u, inl, _ = fsynth.two_view(500, 0.6, 0.0, 0.5, seed=31)
    d = ref.fds(u, cases.f_of(cases.true_f(31)[0]))
    assert np.median(d[inl]) < 1.0 and np.median(d[~inl]) > 100.0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_conditions_of_the_pair_counts(n):
    """the plane-and-parallax candidates of a planar scene: a pair of equal indices gives a NaN matrix and counts 0; pairs of true
    off-plane inliers recover the epipolar geometry (large counts), so the counts are not all alike"""
    uN, us, H, Ht = cases.off_plane_scene(n, 40 + n)
    pairs = cases.pair_block(n, 64, n, True)
    Fs = ref.rfth_candidates(us, pairs, Ht)
    c = ref.count_pairs(uN, us, pairs, Ht, 2 * cases.TH)
    eq = pairs[:, 0] == pairs[:, 1]
    assert eq.any() and np.isnan(Fs[eq]).all() and not np.any(c[eq])
    assert np.isfinite(Fs[~eq]).all()
    if n >= 255:
        assert c.max() > n // 4 and len(np.unique(c)) > 4
