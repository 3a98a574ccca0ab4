"""-m gpu: orientation and description OFF the default mods_describe_params - every SIFT kernel form, the extraction branches only
other patch sizes reach, desc_mrSize beyond the border filter's box, orient_kernel at other patch sizes / mrSizes / thresholds, the
8-bit sampling forms at those settings, a live context taken through a sequence of patch sizes (eagerly and with graph replay), and
the refusals - against the composed CPU reference of tests/describe_ref.py, bit for bit over all region fields and all 128 descriptor
bytes.  Every case asserts, with the census of describe_ref (the oracle's region list and the limits read out of the sources), that
its inputs reach the branch it is named for; tests/test_cpu_describe_params.py asserts the same without a GPU."""
import ctypes as C

import numpy as np
import pytest

import describe_ref as dr
import orc
from test_gpu_describe import _assert_regions_equal
from test_gpu_describe_u8_keys import _tap_boundaries

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _reference(name, img, keys, par):
    """the reference of a call, computed once per (case, parameters): orientation per orientation setting, patches per extraction
    setting, descriptors per descriptor setting"""
    ori_key = (name,) + tuple(par[f] for f in ("ori_mrSize", "ori_patchSize", "ori_maxAngles", "ori_threshold", "ori_halfMode"))
    regs = _cached(("regs",) + ori_key, lambda: dr.oriented(img, keys, par))
    patch_key = ori_key + tuple(par[f] for f in ("desc_mrSize", "desc_patchSize", "photoNorm", "fastExtraction"))
    patches = _cached(("patches",) + patch_key, lambda: dr.patches_of(img, regs, par))
    return _cached(("desc",) + patch_key + (par["rootSift"], par["maxBinValue"], par["halfDesc"]), lambda: dr.describe_patches(regs, patches, par))


def _run(pkg, ctx, img, keys, par, want):
    got = ctx.orient_describe(img, keys, dr.to_struct(pkg, par), max_out=4 * len(keys) + 1)
    if par["halfDesc"]:
        _assert_regions_equal(got, want[0])
        half = ctx.regions_fetch_half(0)
        _assert_regions_equal(half, want[1])
        assert np.all(half["desc"][:, 64:] == 0) and (len(half) <= 2 or half["desc"][:, :64].any())     # (2: the constant patches)
    else:
        _assert_regions_equal(got, want)
    return got


# ---- A. SIFT kernel forms ------------------------------------------------------------------------------------------------------
FORM_VARIANTS = [(ps, dict(rootSift=root)) for ps in sorted(dr.SIFT_FORMS) for root in (1, 0)]
FORM_VARIANTS += [(ps, v) for ps in (39, 43, 63) for v in (dict(photoNorm=0), dict(maxBinValue=0.05), dict(maxBinValue=1.0))]
FORM_VARIANTS += [(ps, dict(halfDesc=1)) for ps in (41, 45, 47)]


@pytest.mark.parametrize("ps,variant", FORM_VARIANTS, ids=lambda v: str(v) if isinstance(v, int) else "-".join("%s=%s" % kv for kv in v.items()))
def test_sift_kernel_forms(pkg, ps, variant):
    """desc_patchSize 9 (the minimum), 39 and 41 (the last sizes of sift_wave2_kernel<16>), 43 and 45 (both sizes of the 18-column form),
    47 (the first size of the block-per-region sift_kernel) and 63 (the maximum), with RootSIFT and with plain SIFT; one size per
    form without the photometric normalisation and with maxBinValue 0.05 and 1.0 (39, 43, 63), and with the half descriptor (41, 45,
    47).  Keys: the detector's on a texture with two constant squares, and - in a second call on the same context, whose orientation
    window (mrSize 8) reaches past the squares - a key on the all-0 and one on the all-255 square, whose patches are constant."""
    img, (det, flat) = dr.forms_image(), dr.forms_keys()
    assert dr.sift_form(ps) == dr.SIFT_FORMS[ps]
    par = dr.params(desc_patchSize=ps, **variant)
    flat_par = dict(par, ori_mrSize=dr.FLAT_ORI_MRSIZE)
    want, want_flat = _reference("forms", img, det, par), _reference("flat", img, flat, flat_par)
    n = len(want[0] if par["halfDesc"] else want)
    assert n >= 100 and len(want_flat[0] if par["halfDesc"] else want_flat) == 2
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        _run(pkg, ctx, img, det, par, want)
        _run(pkg, ctx, img, flat, flat_par, want_flat)
    finally:
        ctx.close()


@pytest.mark.parametrize("ps", [29, 31, 33])
def test_wave_form_around_the_photometric_chunk_size(pkg, ps):
    """sift_wave2_kernel stages the photometric sums through a chunk of 8 x 68 floats that shares LDS with the wave's pixel row of
    8 * ps + 20 float2: below ps = 32 the chunk is the larger one (at 31 by four floats, which were the wave's means).  The last two
    sizes below that limit and the first one above it, photoNorm on."""
    assert dr.wave_chunk_limit() == 31 and dr.sift_form(ps) == "wave16"
    img, (det, _) = dr.forms_image(), dr.forms_keys()
    par = dr.params(desc_patchSize=ps)
    want = _reference("forms", img, det, par)
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        _run(pkg, ctx, img, det, par, want)
    finally:
        ctx.close()


# ---- B. extraction limits as functions of the patch size -----------------------------------------------------------------------
def _limits_census(ps):
    img, keys, par, limits, sizes = dr.limits_case(ps)
    h, w = img.shape
    want = _reference("limits%d" % ps, img, keys, par)
    cen = dr.census(want, w, h, par)
    print("ps %d: limits %s, sizes %s, census %s" % (ps, limits, sizes, cen))
    assert set(sizes) <= set(dr._p2(want, ps, par["desc_mrSize"]).tolist())
    dr.assert_census(cen, ["direct", "lds", "fused"] + (["lds_sent_to_hbm"] if ps in (9, 21) else []))
    if ps == 9:
        assert _tap_boundaries(9)[0] in limits
    return img, keys, par, want


@pytest.mark.parametrize("ps", [9, 21, 41, 63])
def test_extraction_limits(pkg, ps):
    """Both window sizes at every limit of the extraction that a 640 x 480 image has room for - the direct branch (P2 = 5 at ps = 9,
    27 at ps = 63), the launches of extract_small_kernel, the row counts of big_fused_kernel, and at ps = 9 and 21 the tap limit that
    sends a window of the LDS tier's sizes to the HBM tier (lds_tier = ... && n_tap <= 32; blur_table_kernel's early return) - each
    at the centre and next to a border."""
    img, keys, par, want = _limits_census(ps)
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        _run(pkg, ctx, img, keys, par, want)
    finally:
        ctx.close()


def _tap_limits_census():
    img, keys, par, limits, sizes = dr.tap_limits_case()
    want = _reference("taps", img, keys, par)
    cen = dr.census(want, 1200, 1200, par)
    print("limits %s, sizes %s, census %s" % (limits, sizes, cen))
    assert sorted(dr._p2(want, 9, par["desc_mrSize"]).tolist()) == sorted(sizes * 2)
    dr.assert_census(cen, ["phase_by_taps", "phase_by_size", "taps_from_slab"])
    assert sum(cen["fused"]) >= 2
    return img, keys, par, want


def test_tap_limits_ps9(pkg):
    """ps = 9, desc_mrSize = 12, 1200 x 1200: windows of 321 | 323 px (n_tap on either side of BIG_FUSE_TAPS: the second takes the
    sample / row-pass / col-res kernels below BIG_FUSE_P2 because big_is_fused is false) and of 1023 | 1025 | 1027 px (n_tap on
    either side of TAPS_LDS: the row pass reads its taps from the slab)."""
    img, keys, par, want = _tap_limits_census()
    ctx = pkg.Context(0, 1200, 1200, 1)
    try:
        _run(pkg, ctx, img, keys, par, want)
    finally:
        ctx.close()


# ---- C. desc_mrSize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mr", [3.0, 5.1962, 12.0])
def test_desc_mrsize(pkg, mr):
    """desc_mrSize 3, the default and 12 at ps = 41.  At 12 - beyond the 6 * sqrt(3) of the border filter's box - every window
    reaches past the box the filter tested: keys beside all four borders, in the LDS tier, the fused tier and the sample tier,
    read outside the image."""
    img, keys, par = dr.mrsize_case(mr)
    h, w = img.shape
    want = _reference("mrsize%g" % mr, img, keys, par)
    cen = dr.census(want, w, h, par)
    print("mrSize %g: %d regions, census %s" % (mr, len(want), cen))
    assert len(want) >= 50
    if mr == 12.0:
        assert all(cen[b][0] >= 4 for b in ("lds", "fused", "phase_by_size")), cen
    ctx = pkg.Context(0, w, h, 1)
    try:
        _run(pkg, ctx, img, keys, par, want)
    finally:
        ctx.close()


def test_fast_extraction_at_another_mrsize(pkg):
    """fastExtraction = 1 at ps = 33 and mrSize = 3.7: 2 * int(mrSize * s) + 1"""
    img, keys = dr.texture(640, 480, 45), dr.detected(640, 480, 45, 8)
    par = dr.params(desc_patchSize=33, desc_mrSize=3.7, fastExtraction=1)
    want = _reference("fast", img, keys, par)
    assert len(want) >= 100 and len(set((2 * (3.7 * want["s"]).astype(int) + 1).tolist())) >= 8
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        _run(pkg, ctx, img, keys, par, want)
    finally:
        ctx.close()


# ---- D. orientation ------------------------------------------------------------------------------------------------------------
def _orientation_case(pkg, par, name="ori"):
    img, keys = dr.texture(640, 480, 49), dr.orientation_keys()
    want = _reference(name, img, keys, par)
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        _run(pkg, ctx, img, keys, par, want)
    finally:
        ctx.close()
    return keys, want


@pytest.mark.parametrize("ori_mr", [3.7, 5.1962, 8.0])
@pytest.mark.parametrize("ori_ps", [8, 33, 34, 48])
def test_orient_kernel_patch_size_and_mrsize(pkg, ori_ps, ori_mr):
    """orient_kernel - the kernel that samples the image - at ori_patchSize 8 (the minimum), 33 (33 * 31 = 1023 votes: the last size
    with 16-bit vote keys), 34 (the first with 32-bit keys) and 48 (the maximum), at ori_mrSize 3.7 and 5.1962 (both truncated by
    2 * int(mrSize) + 1) and 8.  Three keys beside each border: at mrSize 8 their orientation windows reach over it."""
    par = dr.params(ori_patchSize=ori_ps, ori_mrSize=ori_mr)
    keys, want = _orientation_case(pkg, par)
    assert len(want) >= 100 and dr.ori_key_bytes(ori_ps) == (2 if ori_ps <= 33 else 4)
    if ori_mr == 8.0:
        border = np.arange(len(keys) - 12, len(keys))
        sides = dr.ori_window_sides(keys, 640, 480, par)[border] & np.isin(border, want["parent"])[:, None]
        assert sides.sum(axis=0).min() >= 2, sides


def test_orientation_thresholds(pkg):
    """ori_threshold 0.5, 0.8f and 0.95 with ori_maxAngles = 3: the number of regions differs between the three"""
    n = []
    for th in (0.5, orc.ORI_TH, 0.95):
        _, want = _orientation_case(pkg, dr.params(ori_maxAngles=3, ori_threshold=th))
        n.append(len(want))
    print("regions per threshold: %s" % n)
    assert n[0] > n[1] > n[2] > 100


@pytest.mark.parametrize("ori_ps", [33, 34])
def test_orientation_half_mode(pkg, ori_ps):
    par = dr.params(ori_patchSize=ori_ps, ori_halfMode=1)
    _, want = _orientation_case(pkg, par)
    _, full = _orientation_case(pkg, dr.params(ori_patchSize=ori_ps))
    assert len(want) >= 100 and not np.array_equal(want["a11"][:50], full["a11"][:50])


# ---- E. the 8-bit sampling forms -----------------------------------------------------------------------------------------------
def _u8_case(name):
    if name == "limits9":
        return _limits_census(9)
    ps = int(name)
    img, (det, _) = dr.forms_image(), dr.forms_keys()
    par = dr.params(desc_patchSize=ps)
    return img, det, par, _reference("forms", img, det, par)


@pytest.mark.parametrize("kernels", [-1, 0])
@pytest.mark.parametrize("name", ["41", "45", "47", "limits9"])
def test_u8_sampling_forms(pkg, name, kernels):
    """one patch size of every SIFT form and the ps = 9 limits through orient_describe_u8, with the library's choice of 8-bit kernels
    and with none: the fp32 result, which is the reference's"""
    img, keys, par, want = _u8_case(name)
    h, w = img.shape
    assert np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255
    c32, c8 = pkg.Context(0, w, h, 1), pkg.Context(0, w, h, 1)
    try:
        c8.set_u8_kernels(kernels)
        got32 = _run(pkg, c32, img, keys, par, want)
        got8 = c8.orient_describe_u8(img.astype(np.uint8), keys, dr.to_struct(pkg, par), max_out=4 * len(keys) + 1)
        _assert_regions_equal(got8, want)
        assert got8.tobytes() == got32.tobytes() and c8.u8_source_calls() == 1
    finally:
        c32.close(); c8.close()


# ---- F. reconfiguring a live context -------------------------------------------------------------------------------------------
SEQUENCE = [dict(desc_patchSize=ps) for ps in (41, 9, 45, 63, 41)] + [dict(ori_patchSize=ps) for ps in (48, 8, 32)]


def test_reconfigure_live_context(pkg):
    """desc_patchSize 41 -> 9 -> 45 -> 63 -> 41 and then (from the 32 of those calls) ori_patchSize -> 48 -> 8 -> 32 on one context (describe_configure uploads the
    masks and the SIFT tables again, launch_blur_table rebuilds its table): every result is the one a fresh context gives, and the
    reference's."""
    img, (det, _) = dr.forms_image(), dr.forms_keys()
    live = pkg.Context(0, 640, 480, 1)
    try:
        for change in SEQUENCE:
            par = dr.params(**change)
            want = _reference("forms", img, det, par)
            got = _run(pkg, live, img, det, par, want)
            fresh = pkg.Context(0, 640, 480, 1)
            try:
                assert fresh.orient_describe(img, det, dr.to_struct(pkg, par)).tobytes() == got.tobytes(), change
            finally:
                fresh.close()
    finally:
        live.close()


def test_reconfigure_with_graph_replay(pkg):
    """The same sequence through detect_describe_dev with mods_ctx_graphs on, every setting three times (2 images of 2048 x 1024:
    the scale space forks, so recordings are replayed): the first call with a setting uploads tables and runs eagerly, a recording is
    made and replayed only behind a call with the same arguments and the same device tables - graph_replays never grows on the
    first call of a setting and does grow on its repeats - and every call gives the eager context's regions."""
    import torch
    w, h, n_img = 2048, 1024, 2
    assert w * h * n_img >= 4 << 20
    batch = np.stack([dr.texture(w, h, 70 + i) for i in range(n_img)])
    t = torch.from_numpy(batch).cuda()
    torch.cuda.synchronize()
    eager, live = pkg.Context(0, w, h, n_img), pkg.Context(0, w, h, n_img, nonblocking=True)
    try:
        live.graphs(True)
        for change in SEQUENCE:
            par = dr.to_struct(pkg, dr.params(**change))
            eager.detect_describe_dev(t.data_ptr(), n_img, w, h, None, par)
            want = [eager.regions_fetch(i) for i in range(n_img)]
            assert all(len(r) > 1000 for r in want) and eager.graph_replays() == 0
            before = live.graph_replays()
            for call in range(3):
                live.detect_describe_dev(t.data_ptr(), n_img, w, h, None, par)
                for i in range(n_img):
                    _assert_regions_equal(live.regions_fetch(i), want[i])
                if call == 0:
                    assert live.graph_replays() == before, (change, "a recording was replayed across a change of the tables")
            print("%s: graph replays %d -> %d" % (change, before, live.graph_replays()))
            assert live.graph_replays() > before, change
    finally:
        eager.close(); live.close()


# ---- G. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(ori_patchSize=7), dict(ori_patchSize=49), dict(desc_patchSize=7), dict(desc_patchSize=40),
                                 dict(desc_patchSize=65)], ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_refused_patch_sizes(pkg, bad):
    """patch sizes outside describe_configure's range: MODS_E_ARG, nothing launched (the slot's regions are what they were), and the
    next default call on the context is the oracle's"""
    img, keys = dr.texture(640, 480, 49), dr.detected(640, 480, 49, 8)
    want = _reference("refusal", img, keys, dr.params())
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        first = _run(pkg, ctx, img, keys[:40], dr.params(), _reference("refusal40", img, keys[:40], dr.params()))
        par, n = dr.to_struct(pkg, dr.params(**bad)), C.c_int(-1)
        a, k = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(keys)
        out = np.zeros(len(k) + 1, pkg.REGION_DTYPE)
        rc = pkg.lib().mods_orient_describe(ctx.h, a.ctypes.data_as(C.c_void_p), 640, 480, 640, k.ctypes.data_as(C.c_void_p), len(k), C.byref(par),
                                            out.ctypes.data_as(C.c_void_p), len(out), C.byref(n))
        assert rc == -2 and b"unsupported patch sizes" in pkg.lib().mods_last_error()      # MODS_E_ARG
        assert n.value == -1 and not out["desc"].any()
        assert ctx.regions_fetch(0).tobytes() == first.tobytes()
        _run(pkg, ctx, img, keys, dr.params(), want)
    finally:
        ctx.close()
