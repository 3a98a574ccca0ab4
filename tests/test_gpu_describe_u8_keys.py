"""-m gpu: the four kernels that gather from the input image (orient_kernel, extract_small_kernel, big_fused_kernel,
big_sample_kernel), in their 8-bit and fp32 forms, against the CPU oracle bit for bit - with keypoints chosen so that every size
class of the extraction tiers, both forms of the tap (window touching the image border or not) and the direct branch are reached
(orient_describe_u8), with the describe options, with strided and unaligned 8-bit input, and through a graph replay."""
import os
import re

import numpy as np
import pytest

import orc
import synth
from test_gpu_describe import _assert_regions_equal
from test_gpu_describe_u8 import _p2, _window_touches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sift_constants():
    """the size limits of the extraction kernels as csrc/sift.hip defines them"""
    src = open(os.path.join(ROOT, "mods-light-zmq_amd", "csrc", "sift.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, pattern
        return int(m[0])
    k = dict(t_lo=one(r"#define EXTRACT_T_LO (\d+)"), t_mid=one(r"#define EXTRACT_T_MID (\d+)"), small_cap=one(r"constexpr int SMALL_CAP = (\d+);"),
             fuse_p2=one(r"#define BIG_FUSE_P2_MAX (\d+)"), fuse_kb=one(r"#define BIG_FUSE_KB (\d+)"),
             fuse_taps=one(r"constexpr int BIG_FUSE_TAPS = (\d+);"), taps_lds=one(r"constexpr int TAPS_LDS = (\d+);"),
             lds_taps=one(r"const bool lds_tier = have && g\.P2 <= k\.p2_hi && n_tap <= (\d+);"))
    # the two launch sites that choose between the wave forms and the block-per-region form of the SIFT kernel
    block = re.findall(r"if \((?:run_sift && )?ps > (\d+)\)", src)
    assert len(block) == 2 and block[0] == block[1], block
    k["sift_block_ps"] = int(block[0])
    assert re.search(r"int r = 64;\s*while \(r > 4 && r \* P2 > budget\) r >>= 1;", src), "big_fuse_rows (csrc/sift.hip) no longer reads as the loop this pattern expects: bring _fuse_rows below and this pattern in line with it"
    assert len(re.findall(r"const int n_tap = [^;]*\(\(int\)\(2\.0 \* 3\.0 \* \(1\.5f \* g\.scale\) \+ 1\.0\)\) \| 1", src)) == 2, "the tap count (csrc/sift.hip) no longer reads as _n_tap below restates it"
    return k


def _fuse_rows(P2, kb):
    """big_fuse_rows (csrc/sift.hip)"""
    r = 64
    while r > 4 and r * P2 > kb * 256:
        r >>= 1
    return r


def _n_tap(P2, ps):
    """taps of the blur of a P2 wide window: ((int)(2.0 * 3.0 * (1.5f * scale) + 1.0)) | 1 with scale = float(P2 - 2) / float(ps)
    (region_geom and the classification, csrc/sift.hip; cv::GaussianBlur's kernel size for sigma = 1.5f * scale)"""
    f32 = np.float32
    scale = f32(P2 - 2) / f32(ps)
    return int(2.0 * 3.0 * float(f32(1.5) * scale) + 1.0) | 1


def _tap_boundaries(ps):
    """the last (odd) P2 whose blur has at most as many taps as each of the three tap limits of csrc/sift.hip allows: the LDS tier's
    staged taps, the fused kernel's, the row pass's taps in LDS"""
    k = _sift_constants()
    out = []
    for lim in (k["lds_taps"], k["fuse_taps"], k["taps_lds"]):
        P2 = 3
        while _n_tap(P2 + 2, ps) <= lim:
            P2 += 2
        out.append(P2)
    return out


def _boundaries(ps=orc.DESC_PATCH):
    """P2 limits between two paths of the extraction, ascending: the direct branch (the largest window DescribeRegions samples
    directly has P2 - 2 <= 0.4 * patch size), the three launches of extract_small_kernel, the row counts of big_fused_kernel, and
    the limit between the fused kernel and big_sample_kernel.  At small patch sizes the tap limits come to lie among them: the
    one that sends a window of the LDS tier's sizes to the HBM tier, the one that sends a window of the fused kernel's sizes to the
    phase kernels (each where it falls below the size limit of the same decision; at the default patch size neither does)."""
    k = _sift_constants()
    f32 = np.float32
    direct = max(P + 2 for P in range(1, 64, 2) if float(f32(P) / f32(ps)) <= 0.4)
    out = [direct + 1, k["t_lo"], k["t_mid"], k["small_cap"]]
    out += [P2 for P2 in range(k["small_cap"] + 1, k["fuse_p2"]) if _fuse_rows(P2, k["fuse_kb"]) != _fuse_rows(P2 + 1, k["fuse_kb"])]
    taps = _tap_boundaries(ps)
    out += [t for t, size_limit in zip(taps[:2], (k["small_cap"], k["fuse_p2"])) if t < size_limit]
    out = sorted(set(out))
    out.append(k["fuse_p2"])
    assert out == sorted(set(out)) and len(out) >= 8, out
    return out


def _sizes_at(boundary):
    """P2 is odd: the last size at or below a limit and the first one above it"""
    last = boundary if boundary % 2 else boundary - 1
    return last, last + 2


def _s_of(P2, mrsize=orc.DESC_MRSIZE):
    """a scale whose description window is P2 wide: P2 = 2 * ceil(s * mrSize) + 3"""
    return ((P2 - 3) // 2 - 0.5) / mrsize


def _fits(boundary, w, h):
    """whether a window of the first size above the limit, at any rotation, has room in the image"""
    return 1.5 * _sizes_at(boundary)[1] < min(w, h)


def _iso_key(base, x, y, s):
    k = base.copy()
    k["a11"] = k["a22"] = 1.0
    k["a12"] = k["a21"] = 0.0
    k["x"], k["y"], k["s"] = x, y, s
    return k


def _oracle(img, keys):
    h, w = img.shape
    regs = orc.regions_from_keys(keys)
    assert len(orc.filter_centres_inside(regs, w, h)) == len(regs)       # (the oracle's `parent` counts the centres inside)
    return orc.describe_rootsift(img, orc.filter_touch_boundary(orc.detect_orientation(img, regs), w, h))


def _border_key(img, base, s, side, ps=orc.DESC_PATCH, mrsize=orc.DESC_MRSIZE, ori=None):
    """An isotropic key of scale s next to one border of the image (side 0 left, 1 top, 2 right, 3 bottom) whose description window
    reaches over the border while the region passes the border filter: the window is 2 - 3 pixels wider than the filter's box, and
    how far either reaches depends on the orientation found at the place, so the place is searched - with the oracle's orientation
    and border filter alone - in quarter-pixel steps away from the border.  ori: the orientation's mrsize and ps, where not the default."""
    h, w = img.shape
    half = np.ceil(s * mrsize)
    # (the border filter's box is DESC_MRSIZE * s wide whatever the description's mrSize: a wider window touches further inside)
    d = np.arange(0.9 * np.ceil(s * min(mrsize, orc.DESC_MRSIZE)), 1.5 * half + 6, 0.25)
    if side == 0:
        x, y = d, np.full_like(d, h / 2 + 0.5)
    elif side == 1:
        x, y = np.full_like(d, w / 2 + 0.5), d
    elif side == 2:
        x, y = w - 1 - d, np.full_like(d, h / 2 + 0.5)
    else:
        x, y = np.full_like(d, w / 2 + 0.5), h - 1 - d
    cand = np.concatenate([_iso_key(base, xi, yi, s) for xi, yi in zip(x, y)])
    r = orc.filter_touch_boundary(orc.detect_orientation(img, orc.regions_from_keys(cand), **(ori or {})), w, h)
    touch, _ = _window_touches(r, w, h, ps, mrsize)
    assert touch.any(), "no place next to border %d where a region of scale %g survives with a touching window" % (side, s)
    i = np.nonzero(touch)[0][0]
    return _iso_key(base, r["x"][i], r["y"][i], s)


def _boundary_keys(img, base, boundaries, ps=orc.DESC_PATCH, mrsize=orc.DESC_MRSIZE, s_shift=0.0, ori=None):
    """both sizes at every limit, once at the image centre and once next to a border (the four borders in turn); s_shift (below 0.5)
    moves s * mrSize inside the interval that gives the same window size"""
    h, w = img.shape
    keys, sizes = [], []
    for b in boundaries:
        for P2 in _sizes_at(b):
            s = _s_of(P2, mrsize) + s_shift / mrsize
            keys.append(_iso_key(base, w / 2.0, h / 2.0, s))
            keys.append(_border_key(img, base, s, len(sizes) % 4, ps, mrsize, ori))
            sizes.append(P2)
    return np.concatenate(keys), sizes


def _coverage(want, w, h, classes):
    """per class (lo < P2 <= hi; the direct branch is the class below the first limit): described regions whose window touches the
    border, and whose window does not"""
    P2 = _p2(want)
    touch, direct = _window_touches(want, w, h)
    rows = []
    for lo, hi in classes:
        m = (P2 > lo) & (P2 <= hi)
        rows.append((lo, hi, int(np.count_nonzero(m & touch)), int(np.count_nonzero(m & ~touch))))
    return rows, int(np.count_nonzero(direct))


def _run_both(pkg, img, keys, want, kernels):
    """orient_describe (fp32) and orient_describe_u8 of the same image and keys: both the oracle's regions, and the same bytes"""
    h, w = img.shape
    assert np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255
    c32, c8 = pkg.Context(0, w, h, 1), pkg.Context(0, w, h, 1)
    try:
        c8.set_u8_kernels(kernels)
        got32 = c32.orient_describe(img, keys)
        got8 = c8.orient_describe_u8(img.astype(np.uint8), keys)
        print("8-bit source calls: 8-bit context %d, fp32 context %d" % (c8.u8_source_calls(), c32.u8_source_calls()))
        assert c8.u8_source_calls() == 1 and c32.u8_source_calls() == 0
        _assert_regions_equal(got32, want)
        _assert_regions_equal(got8, want)
        assert got32.tobytes() == got8.tobytes()
    finally:
        c32.close(); c8.close()


# ---- a. above the fused tier ---------------------------------------------------------------------------------------------------
A_W, A_H = 1121, 1093
B_W, B_H = 641, 481


@pytest.fixture(scope="module")
def above_fused_case():
    """1121 x 1093 (odd width: odd row strides, odd addresses for the 2-byte pair loads): six isotropic keys at the centre around the
    limit of the fused kernel - their windows are 1013 .. 1035 wide and, rotated by the orientation found, reach the border or do
    not - and the keys of the limits whose windows a 641 x 481 image (test_class_boundaries) has no room for."""
    img = synth.texture(A_W, A_H, seed=33)
    base = orc.detect_hessian_affine(img[:300, :300].copy())[:1].copy()
    top = np.concatenate([_iso_key(base, 560.5, 546.5, s) for s in (97.0, 98.5, 99.0, 99.2, 99.5, 100.0)])
    rest = [b for b in _boundaries()[:-1] if not _fits(b, B_W, B_H)]
    assert all(_fits(b, A_W, A_H) for b in rest)
    low, sizes = _boundary_keys(img, base, rest)
    keys = np.concatenate([top, low])
    return img, keys, _oracle(img, keys), rest, sizes


@pytest.mark.parametrize("kernels", [-1, 8, 15])
def test_regions_above_the_fused_tier_u8_and_fp32(pkg, above_fused_case, kernels):
    """Regions of more than 1024 px - big_sample_kernel, whose 8-bit form samples its first pixels here (kernels = 8 and 15) and whose
    checked tap (floorf, border test, zero outside the image) runs for the first time in either type: one such window touches the
    border, others do not - next to one just below the limit (big_fused_kernel, 8 rows per item) and the sizes on both sides of the
    fused kernel's last change of row count, at the centre and next to a border."""
    img, keys, want, rest, sizes = above_fused_case
    bounds = _boundaries()
    limit, below = bounds[-1], bounds[bounds.index(rest[0]) - 1]
    P2 = _p2(want)
    touch, direct = _window_touches(want, A_W, A_H)
    rows, _ = _coverage(want, A_W, A_H, [(lo, hi) for lo, hi in zip([below] + rest, rest + [limit])] + [(limit, 1 << 30)])
    print("P2 of the described regions %s, touching %s; (lo, hi, touching, free) %s" % (P2.tolist(), touch.astype(int).tolist(), rows))
    assert np.count_nonzero((P2 > limit) & touch) >= 1 and np.count_nonzero((P2 > limit) & ~touch) >= 1
    assert np.count_nonzero((P2 <= limit) & (P2 > limit - 16)) >= 1
    assert set(sizes) <= set(P2.tolist()), (sizes, P2)
    assert all(t > 0 and f > 0 for _, _, t, f in rows), rows
    assert not direct.any()
    _run_both(pkg, img, keys, want, kernels)


# ---- b. class boundaries -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundary_case():
    img = synth.texture(B_W, B_H, seed=41)
    base = orc.detect_hessian_affine(img)[:1].copy()
    bounds = [b for b in _boundaries()[:-1] if _fits(b, B_W, B_H)]
    keys, sizes = _boundary_keys(img, base, bounds)
    return img, keys, _oracle(img, keys), bounds, sizes


@pytest.mark.parametrize("kernels", [-1, 15])
def test_class_boundaries(pkg, boundary_case, kernels):
    """One call with the last size of every class of the extraction and the first size of the next one (the limits come from
    csrc/sift.hip: the direct branch, the three launches of extract_small_kernel, the row counts of big_fused_kernel), each at the
    centre of a 641 x 481 image and next to a border: every class has a window that touches the border (checked tap) and one that
    does not, and the direct branch has regions.  A limit whose sizes the image has no room for (an isotropic region of more than
    ~ 0.66 * 481 px is dropped by the border filter wherever it lies) is in test_regions_above_the_fused_tier_u8_and_fp32."""
    img, keys, want, bounds, sizes = boundary_case
    assert len(bounds) >= 6 and bounds + [b for b in _boundaries()[:-1] if not _fits(b, B_W, B_H)] == _boundaries()[:-1]
    P2 = _p2(want)
    # every class that begins or ends at one of the limits: the one below the first limit is the direct branch's
    classes = [(lo, hi) for lo, hi in zip([0] + bounds, bounds + [_sizes_at(bounds[-1])[1]])]
    rows, n_direct = _coverage(want, B_W, B_H, classes)
    print("limits %s, P2 of the described regions %s; (lo, hi, touching, free) %s; direct branch %d" % (bounds, sorted(P2.tolist()), rows, n_direct))
    assert set(sizes) <= set(P2.tolist()), (sizes, P2)
    assert all(t > 0 and f > 0 for _, _, t, f in rows), rows
    assert n_direct >= 1
    _run_both(pkg, img, keys, want, kernels)


# ---- c. describe options -------------------------------------------------------------------------------------------------------
OPTION_CASES = [dict(max_angles=2), dict(max_angles=5), dict(max_angles=3, half_orientation=True), dict(max_angles=2, add_upright=True),
                dict(half_desc=True), dict(fast_extraction=True)]


@pytest.fixture(scope="module")
def options_oracle():
    """the 640 x 480 image of the option cases and the oracle's result per case, computed once for both masks"""
    img = synth.texture(640, 480, seed=37)
    done = {}

    def result(opts):
        key = tuple(sorted(opts.items()))
        if key not in done:
            done[key] = orc.detect_describe(img, **opts)
        return done[key]
    return img, result


@pytest.mark.parametrize("kernels", [-1, 15])
@pytest.mark.parametrize("opts", OPTION_CASES, ids=lambda o: "-".join("%s=%s" % kv for kv in sorted(o.items())))
def test_describe_options_u8(pkg, options_oracle, opts, kernels):
    """maxAngles > 1 (with kernels = 15: the 8-bit orient_kernel with several peaks per keypoint), halfMode, addUpRight, halfDesc and
    fastExtraction with an 8-bit source, once with the shipped choice of kernels and once with all four on the 8-bit image: the
    oracle's regions with the same options, and the fp32 call's bytes."""
    import torch
    w, h = 640, 480
    img, result = options_oracle
    res = result(opts)
    want, nd_want = res[0], res[-1]
    desc = pkg.DescribeParams.default()
    desc.ori_maxAngles = opts.get("max_angles", 1)
    desc.ori_halfMode, desc.addUpRight = int(opts.get("half_orientation", False)), int(opts.get("add_upright", False))
    desc.halfDesc, desc.fastExtraction = int(opts.get("half_desc", False)), int(opts.get("fast_extraction", False))
    t32 = torch.from_numpy(img).cuda()
    t8 = torch.from_numpy(img.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    c32, c8 = pkg.Context(0, w, h, 1), pkg.Context(0, w, h, 1)
    try:
        c8.set_u8_kernels(kernels)
        nd32, nr32 = c32.detect_describe_dev(t32.data_ptr(), 1, w, h, None, desc)
        nd8, nr8 = c8.detect_describe_dev_u8(t8.data_ptr(), 1, w, h, None, desc)
        print("regions %d, 8-bit source calls %d" % (nr8[0], c8.u8_source_calls()))
        assert c8.u8_source_calls() == 1 and c32.u8_source_calls() == 0
        assert nd8[0] == nd_want == nd32[0] and nr8[0] == len(want) == nr32[0] and len(want) > 500
        got32, got8 = c32.regions_fetch(0), c8.regions_fetch(0)
        _assert_regions_equal(got8, want)
        assert got32.tobytes() == got8.tobytes()
        if opts.get("half_desc"):
            half8 = c8.regions_fetch_half(0)
            _assert_regions_equal(half8, res[1])
            assert np.all(half8["desc"][:, 64:] == 0) and half8["desc"][:, :64].any()
            assert c32.regions_fetch_half(0).tobytes() == half8.tobytes()
    finally:
        c32.close(); c8.close()


# ---- d. strided and unaligned input --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_pair():
    w, h = 481, 363
    a, b, _ = synth.pair(w, h, seed=7)
    batch = np.stack([a, b])
    assert np.array_equal(batch, np.round(batch)) and batch.min() >= 0 and batch.max() <= 255
    return w, h, batch, [orc.detect_describe(im) for im in (a, b)]


def _fetch_and_check(ctx, nd, nr, want):
    out = []
    for i, (exp, nd_exp) in enumerate(want):
        assert nd[i] == nd_exp and nr[i] == len(exp) > 100
        got = ctx.regions_fetch(i)
        _assert_regions_equal(got, exp)
        out.append(got.tobytes())
    return out


@pytest.mark.parametrize("kernels", [-1, 15])
def test_u8_rows_with_padding(pkg, odd_pair, kernels):
    """Rows w + 5 bytes apart in HBM, the padding filled with a value no pixel row may pick up: the batch is packed into fp32 by
    u8_rows_to_f32_kernel and described from there (a call whose rows are not packed has no 8-bit source: the count does not rise)
    - the packed call's regions, and the oracle's."""
    import torch
    w, h, batch, want = odd_pair
    padded = np.full((2, h, w + 5), 171, np.uint8)
    padded[:, :, :w] = batch.astype(np.uint8)
    t8 = torch.from_numpy(batch.astype(np.uint8)).cuda()
    tp = torch.from_numpy(padded).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    try:
        ctx.set_u8_kernels(kernels)
        nd, nr = ctx.detect_describe_dev_u8(t8.data_ptr(), 2, w, h)
        packed = _fetch_and_check(ctx, nd, nr, want)
        assert ctx.u8_source_calls() == 1
        nd, nr = ctx.detect_describe_dev_u8(tp.data_ptr(), 2, w, h, stride=w + 5)
        print("8-bit source calls after the packed and the strided call: %d" % ctx.u8_source_calls())
        assert ctx.u8_source_calls() == 1
        assert _fetch_and_check(ctx, nd, nr, want) == packed
    finally:
        ctx.close()


@pytest.mark.parametrize("kernels", [-1, 15])
def test_u8_batch_at_an_odd_address(pkg, odd_pair, kernels):
    """The packed batch one byte into a device allocation: the conversion takes its scalar form (the source is not 4-byte aligned)
    and the batch starts from an odd base, so that the rows whose 2-byte pair loads fall on odd addresses are the others - the
    aligned call's regions, and the oracle's, from a call that did have its 8-bit source."""
    import torch
    w, h, batch, want = odd_pair
    n = batch.size
    t8 = torch.from_numpy(batch.astype(np.uint8)).cuda()
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    off = 1 if buf.data_ptr() % 2 == 0 else 2
    buf[off:off + n].copy_(t8.reshape(-1))
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + off
    assert ptr % 2 == 1
    ctx = pkg.Context(0, w, h, 2)
    try:
        ctx.set_u8_kernels(kernels)
        nd, nr = ctx.detect_describe_dev_u8(t8.data_ptr(), 2, w, h)
        aligned = _fetch_and_check(ctx, nd, nr, want)
        before = ctx.u8_source_calls()
        nd, nr = ctx.detect_describe_dev_u8(ptr, 2, w, h)
        print("8-bit source calls: %d before, %d after the call at the odd address" % (before, ctx.u8_source_calls()))
        assert ctx.u8_source_calls() == before + 1
        assert _fetch_and_check(ctx, nd, nr, want) == aligned
    finally:
        ctx.close()


@pytest.mark.parametrize("kernels", [-1, 15])
def test_orient_describe_u8_rows_with_padding(pkg, odd_pair, kernels):
    """The host entry point with rows w + 5 bytes apart (a view into a wider array whose other columns hold a value no row may pick
    up): staged packed, so the call has its 8-bit source - the packed array's regions, and the oracle's."""
    w, h, batch, _ = odd_pair
    img = batch[0]
    keys = orc.detect_hessian_affine(img)
    want = _oracle(img, keys)
    assert len(want) > 100
    wide = np.full((h, w + 5), 171, np.uint8)
    wide[:, :w] = img.astype(np.uint8)
    view = wide[:, :w]
    assert view.strides == (w + 5, 1)
    ctx = pkg.Context(0, w, h, 1)
    try:
        ctx.set_u8_kernels(kernels)
        packed = ctx.orient_describe_u8(img.astype(np.uint8), keys)
        strided = ctx.orient_describe_u8(view, keys)
        print("8-bit source calls after the packed and the strided host call: %d" % ctx.u8_source_calls())
        assert ctx.u8_source_calls() == 2
        _assert_regions_equal(packed, want)
        _assert_regions_equal(strided, want)
        assert packed.tobytes() == strided.tobytes()
    finally:
        ctx.close()


def test_orient_describe_u8_refuses_what_needs_the_context(pkg):
    """the two argument checks that a context is needed for (the others: tests/test_cpu_host.py)"""
    import ctypes as C
    ctx = pkg.Context(0, 64, 48, 1)
    try:
        keys = np.zeros(1, pkg.AFFKEY_DTYPE)
        with pytest.raises(pkg.ModsError, match="larger than the context"):
            ctx.orient_describe_u8(np.zeros((49, 64), np.uint8), keys)
        par, n, img = pkg.DescribeParams.default(), C.c_int(), np.zeros((48, 64), np.uint8)
        rc = pkg.lib().mods_orient_describe_u8(ctx.h, C.c_void_p(img.ctypes.data), 64, 48, 64, C.c_void_p(keys.ctypes.data), 1 << 30, C.byref(par), None, 0, C.byref(n))
        assert rc == -2 and b"too many keypoints" in pkg.lib().mods_last_error()
        assert ctx.u8_source_calls() == 0
    finally:
        ctx.close()


# ---- e. graph replay -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forked_batches(pkg):
    """Two sets of 16 images of 641 x 411 - the smallest batch of odd width here whose scale space forks onto the side stream
    (w * h * n_img >= 4 << 20, csrc/pyramid.hip), which is what makes a recording replayable - and their regions from eager fp32
    calls."""
    import torch
    w, h, n_img = 641, 411, 16
    assert w * h * n_img >= 4 << 20 and w * h * (n_img - 1) < 4 << 20
    sets = [np.stack([synth.texture(w, h, seed=700 + 20 * j + i) for i in range(n_img)]) for j in range(2)]
    eager = pkg.Context(0, w, h, n_img)
    want = []
    try:
        for im in sets:
            t = torch.from_numpy(im).cuda()
            torch.cuda.synchronize()
            eager.detect_describe_dev(t.data_ptr(), n_img, w, h)
            want.append([eager.regions_fetch(i) for i in range(n_img)])
    finally:
        eager.close()
    assert all(len(r) > 20 for regs in want for r in regs)
    return w, h, n_img, sets, want


@pytest.mark.parametrize("kernels", [-1, 15])
def test_graph_replay_with_an_8bit_source(pkg, forked_batches, kernels):
    """mods_ctx_graphs with the 8-bit entry point: six calls with two image sets copied alternately into one 8-bit device buffer -
    recorded, then replayed, with the 8-bit launches in the recording - give the eager fp32 regions every time; a change of
    mods_ctx_u8_kernels drops the recording (it holds the other form's launches) and the calls after it are right again; so is an
    fp32 call of the same images behind them."""
    import torch
    w, h, n_img, sets, want = forked_batches
    buf8 = torch.from_numpy(sets[0].astype(np.uint8)).cuda()
    buf32 = torch.from_numpy(sets[0]).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, n_img, nonblocking=True)
    try:
        ctx.graphs(True)
        ctx.set_u8_kernels(kernels)

        def call_u8(j):
            buf8.copy_(torch.from_numpy(sets[j].astype(np.uint8))); torch.cuda.synchronize()
            ctx.detect_describe_dev_u8(buf8.data_ptr(), n_img, w, h)
            for i in range(n_img):
                _assert_regions_equal(ctx.regions_fetch(i), want[j][i])
        for call in range(6):
            call_u8(call % 2)
        replays = ctx.graph_replays()
        print("graph replays after six 8-bit calls: %d, 8-bit source calls %d" % (replays, ctx.u8_source_calls()))
        assert replays >= 3 and ctx.u8_source_calls() == 6
        ctx.set_u8_kernels(0)
        for call in range(6, 8):
            call_u8(call % 2)
        print("graph replays after two more with every kernel back on fp32: %d" % ctx.graph_replays())
        # the recording with the 8-bit launches is gone: the first call behind the change is eager, the second one records anew and
        # replays that (+ 1); had the old recording survived, both calls would have replayed it (+ 2)
        assert ctx.graph_replays() == replays + 1
        assert ctx.u8_source_calls() == 8
        buf32.copy_(torch.from_numpy(sets[1])); torch.cuda.synchronize()
        ctx.detect_describe_dev(buf32.data_ptr(), n_img, w, h)
        for i in range(n_img):
            _assert_regions_equal(ctx.regions_fetch(i), want[1][i])
    finally:
        ctx.close()
