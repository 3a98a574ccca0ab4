"""-m gpu: the six kernels behind LO-RANSAC and DEGENSAC (csrc/ransac.hip, csrc/ransac_f.hip), each driven through its production
launch function by a test seam (mods_test_ransac_*) and compared with the fp64 restatement of degensac's formulas in
ransac_score_ref.py, which test_cpu_ransac_score_ref.py anchors to the host code and to the reference's own build.

Comparison: every finite d to the bit, equal NaN and infinity masks (payloads are not compared), J the same way (a model with a
NaN error has a NaN score), counts equal.  No tolerance: fp64 throughout, one rounding per operation, no contraction on either
side, the MSAC sum in correspondence order.  Shapes sit on the edges of the loops: the wave (64), the 256-row score tile, the
128-row and 384-row chunks of the two gain kernels, their switch at 16 / 17 models, one / two gain workgroups at 64 / 65, and a
hypothesis capacity grown past 128."""
import ctypes as C

import numpy as np
import pytest

import fsynth
import ransac_score_cases as cases
import ransac_score_ref as ref
from test_gpu_ransac import make_corr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN mask", np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), (what, "inf mask")
    fin = np.isfinite(want)
    bad = bits(got[fin]) != bits(want[fin])
    assert not bad.any(), (what, int(bad.sum()), got[fin][bad][:4], want[fin][bad][:4])


def assert_round(got, want, what):
    assert_same(got["d"], want["d"], what + ("d",))
    assert_same(got["J"], want["J"], what + ("J",))
    assert np.array_equal(got["I"], want["I"]), (what, "I", got["I"], want["I"])
    assert np.array_equal(got["Isym"], want["Isym"]), (what, "Isym", got["Isym"], want["Isym"])


def h_round(pkg, u, models, etype, do_sym, th, errs=None):
    """one seam round against the reference; errs caches the reference's (d, s) per error type for the records the kernel saw"""
    got = pkg.ransac_test_score_h(u, models, etype, do_sym, th, cases.H_CHECK_COEF * th)
    assert np.array_equal(bits(got["h"]), bits(models)) and np.array_equal(bits(got["Hinv"]), bits([ref.hinv_of(h) for h in models]))
    errs = {} if errs is None else errs
    if "rec" in errs:
        assert np.array_equal(bits(got["H1"]), bits(errs["rec"][2]))
    else:
        errs["rec"] = (got["h"], got["Hinv"], got["H1"])
    if etype not in errs:
        errs[etype] = ref.errors_h(u, errs["rec"], etype)
    want = ref.scores(*errs[etype], do_sym, th, cases.H_CHECK_COEF * th)
    assert_round(got, want, ("H", len(u), len(models), etype, do_sym, th))
    return got


def f_round(pkg, u, models, etype, do_sym, th, errs=None):
    got = pkg.ransac_test_score_f(u, models, etype, do_sym, th, cases.F_CHECK_COEF * th)
    errs = {} if errs is None else errs
    if etype not in errs:
        errs[etype] = ref.errors_f(u, models, etype)
    want = ref.scores(*errs[etype], do_sym, th, cases.F_CHECK_COEF * th)
    assert_round(got, want, ("F", len(u), len(models), etype, do_sym, th))
    return got


@pytest.mark.parametrize("ln,n", cases.shapes(cases.H_NS))
def test_homography_score_and_gain(pkg, ln, n):
    """ransac_score_kernel + ransac_gain_few_kernel (n <= 16) / ransac_gain_kernel through gpu_score: all three error types with
    and without the symmetric check at th = 16, th equal to one of the reference's own errors, th = 0, th = 1e308"""
    u = cases.h_corr(ln, 7 + ln)
    models, _ = cases.h_models(u, n, ln)
    errs = {}                                                # (the records come back with the first round, which is at th = 16)
    for etype, do_sym, th_kind in cases.rounds(ln, n, (0, 1, 2)):
        if th_kind == "equal" and etype not in errs:
            errs[etype] = ref.errors_h(u, errs["rec"], etype)
        h_round(pkg, u, models, etype, do_sym, cases.round_th(th_kind, errs.get(etype, (None,))[0], ln), errs)


@pytest.mark.parametrize("ln,n", cases.shapes(cases.F_NS))
def test_epipolar_score_and_gain(pkg, ln, n):
    """ransacf_score_kernel + ransac_gain_kernel through gpu_score_f"""
    u, F = cases.f_corr(ln, 5 + ln)
    models, _ = cases.f_models(F, n, ln)
    errs = {}
    for etype, do_sym, th_kind in cases.rounds(ln, n, (0, 1)):
        if th_kind == "equal" and etype not in errs:
            errs[etype] = ref.errors_f(u, models, etype)
        f_round(pkg, u, models, etype, do_sym, cases.round_th(th_kind, errs.get(etype, (None,))[0], ln), errs)


def _same_run(a, b):
    assert set(a) == set(b)
    for key in a:
        va, vb = np.asarray(a[key]), np.asarray(b[key])
        assert va.shape == vb.shape and va.tobytes() == vb.tobytes(), key


def test_workspace_reuse_across_rounds_and_runs(pkg):
    """One thread, one workspace: a long and wide homography round (len past the 16384 floor of the row capacity, two gain
    workgroups), then a short narrow one (stale gain rows and columns), an epipolar round (the other record size in the same
    hypothesis buffer), a homography round again - each equal to the reference - with a whole exp_ransacHcustom and a whole
    exp_ransacFcustom run in between, which must give what they give on their own."""
    uh = make_corr(700, 0.5, 0.5, 77)
    uf = fsynth.two_view(700, 0.6, 0.0, 0.5, seed=78)[0]
    alone_h = pkg.ransac_h(uh, 16.0, max_sam=5000, err="symm_sum", sym_check=1, seed_time=5)
    alone_f = pkg.ransac_f(uf, 16.0, max_sam=200, err="sampson", sym_check=1, seed_time=5)
    assert alone_h["I"] > 50 and alone_f["I"] > 8

    u1 = cases.h_corr(16385, 3)
    h_round(pkg, u1, cases.h_models(u1, 65, 1)[0], 1, 1, cases.TH)
    _same_run(pkg.ransac_h(uh, 16.0, max_sam=5000, err="symm_sum", sym_check=1, seed_time=5), alone_h)
    u2 = cases.h_corr(100, 4)
    h_round(pkg, u2, cases.h_models(u2, 3, 2)[0], 0, 1, cases.TH)
    u3, F3 = cases.f_corr(300, 6)
    f_round(pkg, u3, cases.f_models(F3, 24, 3)[0], 0, 1, cases.TH)
    _same_run(pkg.ransac_f(uf, 16.0, max_sam=200, err="sampson", sym_check=1, seed_time=5), alone_f)
    u4 = cases.h_corr(300, 8)
    h_round(pkg, u4, cases.h_models(u4, 8, 4)[0], 2, 1, cases.TH)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("k", [1, 7, 2048])
def test_plane_and_parallax_pair_counts(pkg, n, k):
    """ransacf_count_pairs_kernel through gpu_upload_aux and gpu_count_pairs_begin / _end, a block in each of the two slots in
    flight together; one candidate of two equal indices (ec = 0, a NaN matrix) counts 0; limit = 2 th as rFtH passes it"""
    uN, us, _, Ht = cases.off_plane_scene(n, 40 + n)
    k1 = {1: 7, 7: 2048, 2048: 1}[k]
    p0 = cases.pair_block(n, k, 100 * n + k, k > 1)
    p1 = cases.pair_block(n, k1, 100 * n + k + 50, k == 1)
    c0, c1 = pkg.ransac_test_count_pairs(uN, us, Ht, 2 * cases.TH, p0, p1)
    w0, w1 = ref.count_pairs(uN, us, p0, Ht, 2 * cases.TH), ref.count_pairs(uN, us, p1, Ht, 2 * cases.TH)
    assert np.array_equal(c0, w0), (np.flatnonzero(c0 != w0)[:8], c0[c0 != w0][:8], w0[c0 != w0][:8])
    assert np.array_equal(c1, w1), (np.flatnonzero(c1 != w1)[:8], c1[c1 != w1][:8], w1[c1 != w1][:8])
    for p, c in ((p0, c0), (p1, c1)):
        assert not np.any(c[p[:, 0] == p[:, 1]])


@pytest.mark.parametrize("ln", [1, 255, 256, 1023, 1024, 1025, 3000])
@pytest.mark.parametrize("k", [1, 105, 256, 257])
def test_model_counts(pkg, ln, k):
    """ransacf_count_models_kernel through gpu_count_models: COUNT_PARTS = 4 partial counts of 256-row strides (1024 rows a
    sweep), k = 105 models of an innerFH round, 257 past the first capacity; one model with NaN entries counts 0"""
    u, F = cases.f_corr(ln, 9 + ln)
    models, _ = cases.f_models(F, max(k - 1, 1), ln + k)
    if k > 1:
        bad = F.copy()
        bad[4] = np.nan
        models = np.ascontiguousarray(np.vstack([models[:k // 2], bad[None], models[k // 2:]]))
    assert len(models) == k
    got = pkg.ransac_test_count_models(u, models, 2 * cases.TH)
    want = ref.count_models(u, models, 2 * cases.TH)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    if k > 1:
        assert got[k // 2] == 0
    if ln >= 255:
        assert got[0] > ln // 8            # the true F counts the scene's inliers


HDS_T = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
FDS_T = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)


@pytest.mark.parametrize("ln", [128, 129, 384, 385, 2000])
def test_device_scoring_equals_host_scoring_h(pkg, ln):
    """exp_ransacHcustom scores on the host when it is handed a foreign error function.  A callback around the library's own
    HDs / HDsSym / HDsSymMax is foreign to it and computes the same bits, so the host-scored run must take the decisions of the
    GPU-scored one: the same samples, LO runs, rejections and I, and the bits of J, H and the inlier mask.  max_sam ends on and
    one past the batch edges (8, then 64, then 128 samples)."""
    L = pkg.lib()
    u = make_corr(ln, 0.5, 0.5, 900 + ln)
    for err, name in (("sampson", "HDs"), ("symm_sum", "HDsSym"), ("symm_max", "HDsSymMax")):
        fn = getattr(L, name)
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        calls = [0]

        def through(lin, uu, H, p, n, fn=fn, calls=calls):
            calls[0] += 1
            fn(lin, uu, H, p, n)
        cb = HDS_T(through)
        for max_sam in (8, 9, 72, 73, 300):
            for sym in (0, 1):
                dev = pkg.ransac_h(u, 16.0, max_sam=max_sam, err=err, sym_check=sym, seed_time=4321)
                before = calls[0]
                host = pkg.ransac_h(u, 16.0, max_sam=max_sam, err=err, sym_check=sym, seed_time=4321, errfn=cb)
                assert calls[0] > before
                _same_run(dev, host)
                assert dev["samples"] >= 1


@pytest.mark.parametrize("ln", [128, 129, 384, 385, 2000])
def test_device_scoring_equals_host_scoring_f(pkg, ln):
    """the same for exp_ransacFcustom with a callback around FDs, on scenes without a dominant plane; its batches are 8, 16,
    32, 64 ... samples, so max_sam also ends on and one past 24 and 56"""
    L = pkg.lib()
    L.FDs.restype = None
    L.FDs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    u = fsynth.two_view(ln, 0.6, 0.0, 0.5, seed=300 + ln)[0]
    calls = [0]

    def through(uu, F, p, n):
        calls[0] += 1
        L.FDs(uu, F, p, n)
    cb = FDS_T(through)
    for max_sam in (8, 9, 24, 25, 56, 57, 72, 73, 200):
        for sym in (0, 1):
            dev = pkg.ransac_f(u, 16.0, max_sam=max_sam, sym_check=sym, seed_time=4321)
            host = pkg.ransac_f(u, 16.0, max_sam=max_sam, sym_check=sym, seed_time=4321, errfn=cb)
            _same_run(dev, host)
    assert calls[0] > 0
