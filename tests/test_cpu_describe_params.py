"""The reference for orientation + description off the default parameters (tests/describe_ref.py) against the oracle's fixed-parameter
entry points, and the branch census of the GPU cases of tests/test_gpu_describe_params.py from the oracle's region lists alone: the
inputs of every case do reach the kernel form and the branches the case is named for.  No GPU."""
import numpy as np
import pytest

import describe_ref as dr
import orc
import synth
from test_gpu_describe_u8_keys import _boundaries, _n_tap, _sift_constants, _sizes_at, _tap_boundaries


def test_composed_reference_equals_the_fixed_parameter_oracle():
    """at the default parameters: orc.describe_rootsift and orc.detect_describe, bit for bit (and the half descriptors)"""
    w, h = 320, 240
    img = synth.texture(w, h, seed=61)
    keys = orc.detect_hessian_affine(img)
    got = dr.describe(img, keys, dr.params())
    regs = orc.filter_touch_boundary(orc.detect_orientation(img, orc.regions_from_keys(keys)), w, h)
    want = orc.describe_rootsift(img, regs)
    assert len(want) > 100 and got.tobytes() == want.tobytes()
    both, nd = orc.detect_describe(img)
    assert nd == len(keys) and got.tobytes() == both.tobytes()
    full, half, _ = orc.detect_describe(img, half_orientation=True, half_desc=True)
    got_full, got_half = dr.describe(img, keys, dr.params(ori_halfMode=1, halfDesc=1))
    assert got_full.tobytes() == full.tobytes() and got_half.tobytes() == half.tobytes()
    assert not np.array_equal(got_full["a11"], got["a11"][:len(got_full)]) or len(got_full) != len(got)
    fast, _ = orc.detect_describe(img, fast_extraction=True)
    assert dr.describe(img, keys, dr.params(fastExtraction=1)).tobytes() == fast.tobytes()


def test_constants_and_restatements():
    k = _sift_constants()
    assert k["sift_block_ps"] == 45 and k["lds_taps"] == 32 and k["fuse_taps"] == 320 and k["taps_lds"] == 1024
    # spans as csrc/sift.hip's sift_col_span gives them: only 43 and 45 select the 18-column form
    assert [dr.sift_col_span(ps) for ps in (33, 41, 43, 45)] == [13, 15, 17, 18]
    assert {ps: dr.sift_form(ps) for ps in dr.SIFT_FORMS} == dr.SIFT_FORMS
    assert [ps for ps in range(9, 64, 2) if dr.sift_form(ps) == "wave18"] == [43, 45]
    assert dr.wave_chunk_limit() == 31                   # (test_wave_form_around_the_photometric_chunk_size stands next to it)
    assert [dr.ori_key_bytes(ps) for ps in (8, 32, 33, 34, 48)] == [2, 2, 2, 4, 4] and 33 * 31 == 1023
    # the tap limits: never inside their size limits at the default patch size, at P2 = 35 | 323 | 1025 with ps = 9
    assert all(t > lim for t, lim in zip(_tap_boundaries(41), (k["small_cap"], k["fuse_p2"], 4661 - 1)))
    assert [t + 2 for t in _tap_boundaries(9)] == [35, 323, 1025]
    # (in float32 1.5f * scale falls on either side of the integer: the tap count on the two sides of a limit is 2 or 4 apart)
    pairs = [(_n_tap(t, 9), _n_tap(t + 2, 9)) for t in _tap_boundaries(9)]
    print(pairs)
    assert all(a <= lim < b <= lim + 3 and lim - 3 <= a for (a, b), lim in zip(pairs, (k["lds_taps"], k["fuse_taps"], k["taps_lds"])))
    assert _boundaries() == [18, 48, 64, 80, 128, 256, 512, 1024]          # the default list is what it was


@pytest.mark.parametrize("ps", sorted(dr.SIFT_FORMS))
def test_census_sift_forms(ps):
    """A: the detector's keys and the two constant squares reach the form the patch size is named for"""
    img, (det, flat) = dr.forms_image(), dr.forms_keys()
    h, w = img.shape
    regs = dr.oriented(img, det, dr.params())
    flat_regs = dr.oriented(img, flat, dr.params(ori_mrSize=dr.FLAT_ORI_MRSIZE))
    assert dr.sift_form(ps) == dr.SIFT_FORMS[ps] and 100 <= len(regs) <= 400 and len(flat_regs) == 2
    patches = dr.patches_of(img, flat_regs, dr.params(desc_patchSize=ps, photoNorm=0))
    assert np.all(patches[0] == patches[0][0, 0]) and np.all(patches[1] == patches[1][0, 0]) and patches[1].max() > 200 > 1 > patches[0].max()


@pytest.mark.parametrize("ps", [9, 21, 41, 63])
def test_census_extraction_limits(ps):
    """B: both sizes at every limit are described, each class between two limits has a window that touches the border and one
    that does not, and the branches that exist only off the default patch size hold their regions"""
    img, keys, par, limits, sizes = dr.limits_case(ps)
    h, w = img.shape
    regs = dr.oriented(img, keys, par)
    P2 = dr._p2(regs, ps, par["desc_mrSize"])
    assert set(sizes) <= set(P2.tolist()), (sizes, sorted(P2.tolist()))
    cen = dr.census(regs, w, h, par)
    print(ps, limits, cen)
    dr.assert_census(cen, ["direct", "lds", "fused"])
    assert cen["direct"][1] >= 1 and all(min(cen[b]) >= 1 for b in ("lds", "fused"))
    if ps == 9:
        assert _tap_boundaries(9)[0] in limits
        dr.assert_census(cen, ["lds_sent_to_hbm"])
        assert min(cen["lds_sent_to_hbm"]) >= 1
    if ps == 21:
        assert _tap_boundaries(21)[0] in limits
        dr.assert_census(cen, ["lds_sent_to_hbm"])
    if ps == 63:      # the direct branch takes every window up to P = 25
        direct_sizes = [p for p in sizes if p <= 27]
        assert direct_sizes == [27] and _sizes_at(_boundaries(63)[0]) == (27, 29)


def test_census_tap_limits():
    """B, 1200 x 1200: n_tap 319|321 (the fused kernel's taps) and 1023|1025 (the row pass's taps in LDS), both sizes twice"""
    img, keys, par, limits, sizes = dr.tap_limits_case()
    h, w = img.shape
    regs = dr.oriented(img, keys, par)
    P2 = dr._p2(regs, 9, par["desc_mrSize"])
    assert sizes == [321, 323, 1023, 1025, 1027] and sorted(P2.tolist()) == sorted(sizes * 2), (sizes, P2)
    cen = dr.census(regs, w, h, par)
    print(cen)
    assert sum(cen["fused"]) == 2 and sum(cen["phase_by_taps"]) == 4 and sum(cen["phase_by_size"]) == 4 and sum(cen["taps_from_slab"]) == 4
    dr.assert_census(cen, ["phase_by_taps", "phase_by_size", "taps_from_slab"])


@pytest.mark.parametrize("mr", [3.0, 5.1962, 12.0])
def test_census_desc_mrsize(mr):
    img, keys, par = dr.mrsize_case(mr)
    h, w = img.shape
    regs = dr.oriented(img, keys, par)
    cen = dr.census(regs, w, h, par)
    print(mr, len(regs), cen)
    assert 50 <= len(regs) <= 400
    if mr == 12.0:     # windows that reach outside the image in the LDS tier, the fused tier and the sample tier: one per border
        for b in ("lds", "fused", "phase_by_size"):
            assert cen[b][0] >= 4, cen


@pytest.mark.parametrize("ori_mr", [3.7, 5.1962, 8.0])
@pytest.mark.parametrize("ori_ps", [8, 33, 34, 48])
def test_census_orientation(ori_ps, ori_mr):
    """D: the keys beside the borders survive at every setting; at ori_mrSize 8 their orientation windows reach over each border"""
    img, keys = dr.texture(640, 480, 49), dr.orientation_keys()
    par = dr.params(ori_patchSize=ori_ps, ori_mrSize=ori_mr)
    regs = dr.oriented(img, keys, par)
    border = np.arange(len(keys) - 12, len(keys))
    alive = np.isin(border, regs["parent"])
    sides = dr.ori_window_sides(keys, 640, 480, par)[border]
    print(ori_ps, ori_mr, len(regs), alive.sum(), sides.sum(axis=0))
    assert 100 <= len(regs) <= 400
    if ori_mr == 8.0:
        assert (sides & alive[:, None]).sum(axis=0).min() >= 2
    assert dr.ori_key_bytes(ori_ps) == (2 if ori_ps <= 33 else 4)
    assert int(ori_mr) != ori_mr or ori_mr == 8.0        # 3.7 and 5.1962 are truncated by 2 * int(mrSize) + 1


def test_census_orientation_thresholds():
    """D: the three thresholds give three different region counts with ori_maxAngles = 3 (or the axis tests nothing)"""
    img, keys = dr.texture(640, 480, 49), dr.orientation_keys()
    n = [len(dr.oriented(img, keys, dr.params(ori_maxAngles=3, ori_threshold=th))) for th in (0.5, orc.ORI_TH, 0.95)]
    print(n)
    assert n[0] > n[1] > n[2] > 100
