"""-m gpu: the 8-bit images in 16-byte column strips (csrc/u8_strips.hpp) as the third source of the four kernels that gather from
the input image - the copy the conversion launch makes against the numpy restatement of the layout, and the regions sampled from
it against those sampled from the fp32 and from the row-major 8-bit images, byte for byte."""
import numpy as np
import pytest

import orc
import synth
from test_cpu_u8_strips import strips_of
from test_gpu_describe_u8 import P2_CLASSES, RES_FIELDS, _alone_fp32, _assert_same, _collect, _p2, _pinned_pairs, _window_touches  # noqa: F401
from test_gpu_describe_u8_keys import A_H, A_W, _border_key, _iso_key, forked_batches  # noqa: F401

pytestmark = pytest.mark.gpu

FP32, ROW_MAJOR, STRIPS, DEFAULT = 0, 15, 15 << 4, -1      # masks of set_u8_kernels: all four kernels on one source


# ---- the producer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,src_offset", [(481, 363, 0), (250, 170, 0), (481, 363, 1)],
                         ids=["481x363", "250x170-partial-last-strip", "481x363-odd-address"])
def test_strip_copy_of_a_batch(pkg, w, h, src_offset):
    """Two random images through the conversion launch: 481 x 363 - w - 1 a multiple of 15 (the last strip is full, and its 16th
    column is the image's last), h no multiple of 8 (five padding rows per strip) -, 250 x 170 (the last strip has 9 + 1 columns of
    16, six padding rows) and the 481 x 363 batch one byte into the staging area (every 16-byte load at an odd address).  Every byte
    of the copy, the zero padding included - the buffer is filled with ones by a larger batch first."""
    assert (w - 1) % 15 == (0 if w == 481 else 9) and h % 8 != 0
    rng = np.random.default_rng(w + src_offset)
    batch = rng.integers(1, 256, (2, h, w), dtype=np.uint8)
    ctx = pkg.Context(0, 512, 384, 2)
    try:
        ones = ctx.u8_strips_fetch(np.ones((2, 384, 512), np.uint8))
        assert ones[:, :-1, :, :].all() and not ones[:, -1, :, 2:].any()      # (the 35th strip holds the columns 510 and 511)
        got = ctx.u8_strips_fetch(batch, src_offset)
        want = np.stack([strips_of(im, pkg) for im in batch])
        assert got.shape == want.shape
        assert np.array_equal(got, want)
        assert (want == 0).any()
    finally:
        ctx.close()


# ---- the consumers, on what the detector finds ---------------------------------------------------------------------------------
def _regions(pkg, batch, mask):
    import torch
    n, h, w = batch.shape
    ctx = pkg.Context(0, w, h, n)
    try:
        ctx.set_u8_kernels(mask)
        if mask == FP32:
            t = torch.from_numpy(batch).cuda()
            torch.cuda.synchronize()
            nd, nr = ctx.detect_describe_dev(t.data_ptr(), n, w, h)
        else:
            t = torch.from_numpy(batch.astype(np.uint8)).cuda()
            torch.cuda.synchronize()
            nd, nr = ctx.detect_describe_dev_u8(t.data_ptr(), n, w, h)
        return nd, nr, [ctx.regions_fetch(i) for i in range(n)], ctx.u8_source_calls(), ctx.u8_strip_calls()
    finally:
        ctx.close()


@pytest.fixture(scope="module", params=[(481, 363, 5), (250, 170, 4)], ids=["481x363", "250x170"])
def detected(pkg, request):
    """a batch of two images and its regions from an fp32 context and from one with all four kernels on the row-major 8-bit images"""
    w, h, n_classes = request.param
    a, b, _ = synth.pair(w, h, seed=7)
    batch = np.stack([a, b])
    assert np.array_equal(batch, np.round(batch)) and batch.min() >= 0 and batch.max() <= 255
    r32, r8 = _regions(pkg, batch, FP32), _regions(pkg, batch, ROW_MAJOR)
    assert r32[3:] == (0, 0) and r8[3:] == (1, 0)
    return w, h, n_classes, batch, r32, r8


@pytest.mark.parametrize("mask", [STRIPS, DEFAULT], ids=["all-four-on-strips", "shipped-default"])
def test_regions_from_strips_equal_fp32_and_row_major(pkg, detected, mask):
    """The region arrays of a context with all four kernels on the strips (orient_kernel, the three launches of extract_small_kernel
    with its direct branch, big_fused_kernel; big_sample_kernel runs on an empty list at these sizes, given keypoints reach it
    below) are the bytes of the fp32 context's and of the row-major 8-bit context's; once more with the mask the library ships.
    The coverage is asserted: regions in every P2 class a window of which fits the image - all five at 481 x 363, as in
    tests/test_gpu_describe_u8.py; at 250 x 170 no window of more than 256 pixels has room - and windows that touch the border
    (clamped taps) as well as windows that do not."""
    w, h, n_classes, batch, r32, r8 = detected
    nd, nr, regs, u8_calls, strip_calls = _regions(pkg, batch, mask)
    assert (nd, nr) == r32[:2] == r8[:2]
    assert u8_calls == 1
    if mask == STRIPS:
        assert strip_calls == 1
    seen = np.zeros(n_classes, np.int64)
    n_touch = n_free = 0
    for i in range(2):
        assert len(regs[i]) == nr[i] and len(regs[i]) > 30
        assert regs[i].tobytes() == r32[2][i].tobytes()
        assert regs[i].tobytes() == r8[2][i].tobytes()
        P2 = _p2(regs[i])
        seen += np.array([np.count_nonzero((P2 > lo) & (P2 <= hi)) for lo, hi in P2_CLASSES[:n_classes]])
        touch, _ = _window_touches(regs[i], w, h)
        n_touch += np.count_nonzero(touch); n_free += np.count_nonzero(~touch)
    print("%d x %d, mask %d: regions per P2 class %s, windows touching the border %d, not touching %d, strip calls %d"
          % (w, h, mask, seen.tolist(), n_touch, n_free, strip_calls))
    assert (seen > 0).all(), seen
    assert n_touch > 0 and n_free > 0


# ---- given keypoints -----------------------------------------------------------------------------------------------------------
def _three_sources(pkg, img, keys):
    """orient_describe (fp32) and orient_describe_u8 with all four kernels on the row-major 8-bit image and on the strips"""
    h, w = img.shape
    out = []
    for mask in (FP32, ROW_MAJOR, STRIPS):
        ctx = pkg.Context(0, w, h, 1)
        try:
            ctx.set_u8_kernels(mask)
            out.append(ctx.orient_describe(img, keys) if mask == FP32 else ctx.orient_describe_u8(img.astype(np.uint8), keys))
            assert ctx.u8_strip_calls() == (1 if mask == STRIPS else 0)
        finally:
            ctx.close()
    return out


@pytest.fixture(scope="module")
def seam_image():
    img = synth.texture(250, 170, seed=51)
    return img, orc.detect_hessian_affine(img)[:1].copy()


def test_taps_at_strip_seams_and_line_boundaries(pkg, seam_image):
    """Isotropic keys at whole-pixel centres: direct-branch regions (P2 = 7: the 41 x 41 patch is sampled at 0.12 px steps, so every
    tap lies within three pixels of the centre) centred on x = 13, 14, 15 (mod 15) and y = 7, 8 (mod 8) - the last own column of a
    strip, the shared one, the first of the next; the last row of a 128-byte line and the first of the next - and windows of
    19 x 19 and 45 x 45 there, which cover every residue.  Not every key becomes a region (the orientation stage drops some): the
    test asserts that the regions it compares still have all six residues in the direct branch and in the windows."""
    img, base = seam_image
    keys = []
    for s in (0.3, 1.5, 4.0):
        for x in (28, 29, 30, 58, 59, 60, 133, 134, 135):
            for y in (39, 40, 63, 64, 87, 88):
                keys.append(_iso_key(base, float(x), float(y), s))
    keys = np.concatenate(keys)
    assert {int(k["x"]) % 15 for k in keys} == {13, 14, 0} and {int(k["y"]) % 8 for k in keys} == {7, 0}
    g32, g8, gs = _three_sources(pkg, img, keys)
    P2 = _p2(gs)
    _, direct = _window_touches(gs, 250, 170)
    print("regions %d of %d keys, P2 %s, direct branch %d" % (len(gs), len(keys), sorted(set(P2.tolist())), np.count_nonzero(direct)))
    for group in (direct, ~direct):
        assert {int(x) % 15 for x in gs["x"][group]} == {13, 14, 0} and {int(y) % 8 for y in gs["y"][group]} == {7, 0}
    assert gs.tobytes() == g8.tobytes() and gs.tobytes() == g32.tobytes()


def test_taps_clamped_at_the_last_pair(pkg, seam_image):
    """windows that reach over the right and the bottom border: the checked tap clamps its pair to x = w - 2 and y = h - 2 - 250 x 170:
    x = 248 is byte 8 of the last strip, whose bytes 10 .. 15 are padding; y = 168 is the first row of the last line, whose rows
    170 .. 175 are padding"""
    img, base = seam_image
    keys = np.concatenate([_border_key(img, base, s, side) for s in (1.5, 4.0, 7.0) for side in (2, 3)])
    g32, g8, gs = _three_sources(pkg, img, keys)
    touch, _ = _window_touches(gs, 250, 170)
    print("regions %d, windows over the border %d" % (len(gs), np.count_nonzero(touch)))
    assert len(gs) >= 6 and np.count_nonzero(touch) >= 6
    assert gs.tobytes() == g8.tobytes() and gs.tobytes() == g32.tobytes()


def test_region_above_1024_from_strips(pkg):
    """1121 x 1093: isotropic keys at the centre whose windows are 1013 .. 1035 wide - above 1024 big_sample_kernel samples them (its
    strip form runs nowhere else), below it big_fused_kernel at its smallest row count"""
    img = synth.texture(A_W, A_H, seed=33)
    base = orc.detect_hessian_affine(img[:300, :300].copy())[:1].copy()
    keys = np.concatenate([_iso_key(base, 560.5, 546.5, s) for s in (97.0, 98.5, 99.0, 99.2, 99.5, 100.0)])
    g32, g8, gs = _three_sources(pkg, img, keys)
    P2 = _p2(gs)
    print("P2 of the described regions %s" % P2.tolist())
    assert (P2 > 1024).any() and (P2 <= 1024).any()
    assert gs.tobytes() == g8.tobytes() and gs.tobytes() == g32.tobytes()


def test_graph_replay_from_strips(pkg, forked_batches):
    """mods_ctx_graphs with all four kernels on the strips: the conversion launch, which makes the strips, runs ahead of the recorded
    chain in every call, the recording holds the strip forms' launches and the strip copy's address is part of its key - six calls
    with two image sets alternating in one device buffer give the eager fp32 regions every time, and a change of the mask drops the
    recording."""
    import torch
    w, h, n_img, sets, want = forked_batches
    buf8 = torch.from_numpy(sets[0].astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, n_img, nonblocking=True)
    try:
        ctx.graphs(True)
        ctx.set_u8_kernels(STRIPS)

        def call_u8(j):
            buf8.copy_(torch.from_numpy(sets[j].astype(np.uint8))); torch.cuda.synchronize()
            ctx.detect_describe_dev_u8(buf8.data_ptr(), n_img, w, h)
            for i in range(n_img):
                assert ctx.regions_fetch(i).tobytes() == want[j][i].tobytes()
        for call in range(6):
            call_u8(call % 2)
        replays = ctx.graph_replays()
        print("graph replays after six calls from strips: %d, strip calls %d" % (replays, ctx.u8_strip_calls()))
        assert replays >= 3 and ctx.u8_strip_calls() == 6
        ctx.set_u8_kernels(ROW_MAJOR)
        for call in range(6, 8):
            call_u8(call % 2)
        assert ctx.graph_replays() == replays + 1 and ctx.u8_strip_calls() == 6 and ctx.u8_source_calls() == 8
    finally:
        ctx.close()


def test_pipeline_batches_from_strips(pkg):
    """Two 320 x 240 pairs through a pipeline whose worker has all four kernels on the strips: batches of 8-bit pairs give what the
    same pairs give as fp32, and every such batch had its strip copy."""
    w, h = 320, 240
    pin32, pin8 = _pinned_pairs(pkg, w, h, (7, 8))
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), 1, 1, 2)
    try:
        pipe.set_u8_kernels(STRIPS)
        alone = _alone_fp32(pkg, pipe, pin32)
        pkg.ransac_pin_seed(7)
        before, strips_before = pipe.u8_source_calls(), pipe.u8_strip_calls()
        for j in range(5):
            pipe.submit_host(pin8[j % 2].ptr.value, j % 2, u8=True)
        _assert_same(_collect(pipe, 5), [alone[j % 2] for j in range(5)])
        n, ns = pipe.u8_source_calls() - before, pipe.u8_strip_calls() - strips_before
        print("8-bit batches %d, with a strip copy %d" % (n, ns))
        assert 3 <= n <= 5 and ns == n
    finally:
        pipe.close()
        for b in pin32 + pin8:
            b.close()
