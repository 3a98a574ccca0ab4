"""-m gpu parity tests of the detector on tied, periodic and saturating images (tests/degenerate.py): the raw NMS hit list, the
localised candidates and the keypoints IN LIST ORDER against the CPU oracle, bit for bit.  tests/test_cpu_degenerate.py holds the
images to what they are here for: nms4_kernel's mid-level flush (a), bit-equal responses under the response sort (b, c), plateaux
and singular localisations (d), several images per launch (e), the hit list's overflow (f, the last case of the file) and
responses that overflow to +-inf and NaN (g)."""
import numpy as np
import pytest

import degenerate as dg
import orc
import synth
from degenerate import LATTICE_SEED
from test_gpu_detect import _assert_keys_equal

pytestmark = pytest.mark.gpu


def _assert_stages_equal(ctx, b, img, po, keys):
    """image slot b of the context's last detection against the oracle on img: raw hits, candidates, keys in list order"""
    cand_want, raw_want = orc.Pyramid(img, po).candidates()
    hits, count = ctx.pyramid_nms_hits(b)
    assert count == len(raw_want) and len(hits) == count
    hits = hits[np.lexsort((hits[:, 3], hits[:, 2], hits[:, 1], hits[:, 0]))]
    assert np.array_equal(hits, raw_want), "raw NMS hits differ"
    cand = ctx.pyramid_candidates(b)
    cand = cand[np.lexsort((cand["c0"], cand["r0"], cand["level"], cand["octave"]))]
    assert len(cand) == len(cand_want)
    for f in cand_want.dtype.names:
        assert np.array_equal(cand[f], cand_want[f]), "candidate field %s differs" % f
    want = orc.detect_hessian_affine(img, po)
    _assert_keys_equal(keys, want)        # not sorted: the order of equal responses is part of the contract
    return raw_want, cand_want, want


def _detect_and_compare(pkg, img, det="hessian", **sel):
    h, w = img.shape
    ctx = pkg.Context(0, w, h, 1)
    try:
        keys = ctx.detect_hessian_affine(img, dg.params(pkg, det, **sel))
        return _assert_stages_equal(ctx, 0, img, dg.params(orc, det, **sel), keys)
    finally:
        ctx.close()


# ---- (a) more than 768 in-plane extrema per wave and level: nms4_kernel empties its list in the middle of a level
@pytest.mark.parametrize("w,h", [(512, 96), (500, 64)])
@pytest.mark.parametrize("name", ["dots", "lattice"])
def test_flush_of_the_wave_list(pkg, name, w, h):
    img = dg.dots(w, h, 3, 255) if name == "dots" else dg.tile_lattice(w, h, 3, 255, LATTICE_SEED)
    raw, cand, _ = _detect_and_compare(pkg, img, mode=2, reg=100000)
    assert name == "dots" or len(cand) >= 100


# ---- (b) thousands of keys with bit-equal |response|, extrema on every seam of the NMS tiling
@pytest.mark.parametrize("det,P,w", [("hessian", 6, 500),     # four columns per lane; last block of 4 columns (500 = 2 * 248 + 4)
                                     ("hessian", 6, 501),     # one column per lane (width no multiple of 4)
                                     ("dog", 8, 500),
                                     ("hessian", 7, 500)])    # 248 = 3 mod 7: other residues on the block seams than P = 6 (248 = 2 mod 6)
def test_ties_in_the_response_order(pkg, det, P, w):
    _, _, want = _detect_and_compare(pkg, dg.checker(w, 300, P, 255.0), det)
    assert len(want) >= 1000 and dg.shared_response_fraction(want) >= 0.9


# ---- (c) responses near 1e-5, thresholds 0, the cuts of modes 1-4 inside runs of equal responses, cell collisions
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_small_magnitudes_and_cuts_inside_ties(pkg, mode):
    img = dg.checker(500, 300, 6, 1.0)
    ctx = pkg.Context(0, 500, 300, 1)
    try:
        for reg, rel_th, rel_n in ((300, 0.02, 0.25), (5000, 0.5, 1.0), (0, 0.0, 0.0)):   # test_keypoint_selection_modes' triples
            sel = dict(mode=mode, reg=reg, rel_th=rel_th, rel_n=rel_n)
            keys = ctx.detect_hessian_affine(img, dg.params(pkg, **sel))
            raw, cand, _ = _assert_stages_equal(ctx, 0, img, dg.params(orc, **sel), keys)
            assert len(cand) < len(raw)
    finally:
        ctx.close()


# ---- (d) images constant along an axis: every pixel of a ridge is a 3x3x3 extremum, every localisation a singular system
@pytest.mark.parametrize("det", ["dog", "harris"])
@pytest.mark.parametrize("w", [500, 498])
@pytest.mark.parametrize("vertical", [True, False], ids=["vertical", "horizontal"])
def test_plateaux(pkg, det, w, vertical):
    raw, cand, want = _detect_and_compare(pkg, dg.stripes(w, 300, 12, 255.0, vertical), det)
    if det == "dog":
        assert len(raw) > 20000 and len(cand) == 0 and len(want) == 0


@pytest.mark.parametrize("vertical", [True, False], ids=["vertical", "horizontal"])
def test_zero_response_gives_no_hit(pkg, vertical):
    """stripes of period 8 under the Hessian: Lxx * Lyy - Lxy^2 is exactly 0 everywhere"""
    raw, cand, want = _detect_and_compare(pkg, dg.stripes(500, 300, 8, 255.0, vertical))
    assert len(raw) == 0 and len(want) == 0


# ---- (g) responses that overflow: +-inf beside +-inf in the neighbouring LEVELS (a hit unless a neighbour is strictly beyond it:
# nms_other_planes' comparisons are strict), NaN neighbours under nms4_kernel's fmaxf / fminf form, inf and NaN systems in localize_kernel
@pytest.mark.parametrize("w", [252, 253])     # four columns per lane, one column per lane
def test_saturated_responses_tie_across_levels(pkg, w):
    raw, cand, want = _detect_and_compare(pkg, dg.checker(w, 100, 6, 1e25))
    assert len(raw) > 5000 and len(cand) == 0 and len(want) == 0


# ---- (e) several images per launch: blockIdx.z planes and per-image counters, rank_sort_kernel (more than 4 images)
def _batch(pkg, imgs, det):
    import torch
    h, w = imgs[0].shape
    ctx = pkg.Context(0, w, h, len(imgs))
    try:
        t = torch.from_numpy(np.stack(imgs)).cuda()
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), len(imgs), w, h, dg.params(pkg, det))
        return [_assert_stages_equal(ctx, b, img, dg.params(orc, det), got[b]) for b, img in enumerate(imgs)]
    finally:
        ctx.close()


def test_batch_of_six_sorts_ties_in_lds(pkg):
    imgs = [np.ascontiguousarray(dg.checker(504, 300, 6, 255.0)[:, s:s + 500]) for s in range(5)] + [synth.texture(500, 300, seed=31)]
    res = _batch(pkg, imgs, "hessian")
    assert all(1000 <= len(want) <= 16384 for _, _, want in res[:5])     # rank_sort_kernel's range
    assert len(res[5][2]) > 100


def test_batch_of_two_counts_ranks(pkg):
    res = _batch(pkg, [dg.stripes(500, 300, 12, 255.0, True), synth.texture(500, 300, seed=32)], "dog")
    assert len(res[0][0]) > 20000 and len(res[0][2]) == 0 and len(res[1][2]) > 100


# ---- (f) more hits than the list holds.  The last case of the file: the designed error path, every consumer of the list clamps its
# count to the capacity (nms_compact_kernel's slot test, localize / accept / omap_reset_kernel's n)
def test_hit_list_overflow_is_reported_and_survived(pkg):
    w, h = 640, 512
    img = dg.stripes(w, h, 12, 255.0, True)
    _, raw_want = orc.Pyramid(img, dg.params(orc, "dog")).candidates()
    assert len(raw_want) > 65536
    ctx = pkg.Context(0, w, h, 1)
    try:
        with pytest.raises(pkg.ModsError, match="NMS hit list overflow"):
            ctx.detect_hessian_affine(img, dg.params(pkg, "dog"))
        hits, count = ctx.pyramid_nms_hits(0)
        assert count == len(raw_want) and len(hits) == 65536
        pack = lambda a: ((a[:, 0].astype(np.int64) * 8 + a[:, 1]) << 40) | (a[:, 2].astype(np.int64) << 20) | a[:, 3]
        got = pack(hits)
        assert len(np.unique(got)) == len(got) and np.isin(got, pack(raw_want)).all()
        tex = synth.texture(w, h, seed=41)
        for det in ("hessian", "dog"):
            keys = ctx.detect_hessian_affine(tex, dg.params(pkg, det))
            _, _, want = _assert_stages_equal(ctx, 0, tex, dg.params(orc, det), keys)
            assert len(want) > 100
    finally:
        ctx.close()
