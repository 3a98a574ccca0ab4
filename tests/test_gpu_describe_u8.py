"""-m gpu: orientation and description sampled from the 8-bit images (detect_describe_dev_u8, the pair pipeline's 8-bit batches)
give, to the bit, what the fp32 copy of the same images gives."""
import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu

P2_CLASSES = ((0, 48), (48, 64), (64, 80), (80, 256), (256, 1 << 30))    # lo < P2 <= hi: the three LDS launches, the fused tier's two row counts


def _p2(regions, ps=orc.DESC_PATCH, mrsize=orc.DESC_MRSIZE):
    """side of the sampled window of DescribeRegions, blur margin included (region_geom, csrc/sift.hip; no function of the patch
    size ps, which decides only whether the window is blurred or the patch sampled directly: _window_touches)"""
    return 2 * np.ceil(regions["s"] * mrsize).astype(np.int64) + 1 + 2


def _window_touches(regions, w, h, ps=orc.DESC_PATCH, mrsize=orc.DESC_MRSIZE):
    """interpolateCheckBorders (helpers.cpp:527-549) for the window the description samples: the P2 x P2 window in the region's frame,
    or - regions of at most 0.4 image pixels per patch pixel, which are sampled directly - the patch in the frame times that scale"""
    f32 = np.float32
    P2 = _p2(regions, ps, mrsize)
    scale = (P2 - 2).astype(f32) / f32(ps)
    direct = scale.astype(np.float64) <= 0.4
    n = np.where(direct, ps, P2)
    k = np.where(direct, scale, f32(1)).astype(f32)
    fx, fy = regions["x"].astype(f32), regions["y"].astype(f32)
    a11, a12 = regions["a11"].astype(f32) * k, regions["a12"].astype(f32) * k
    a21, a22 = regions["a21"].astype(f32) * k, regions["a22"].astype(f32) * k
    half = np.ceil(n.astype(f32).astype(np.float64) / 2.0).astype(f32)
    touch = np.zeros(len(regions), bool)
    for sx, sy in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        imx = fx + (f32(sx) * half) * a11 + (f32(sy) * half) * a12
        imy = fy + (f32(sx) * half) * a21 + (f32(sy) * half) * a22
        touch |= (np.floor(imx) <= 0) | (np.floor(imy) <= 0) | (np.ceil(imx) >= w - 2) | (np.ceil(imy) >= h - 2)
    return touch, direct


@pytest.mark.parametrize("kernels", [-1, 15])
def test_u8_entry_point_equals_fp32(pkg, kernels):
    """A batch of two 481 x 363 images - odd width and height: odd row strides, so the 2-byte pixel-pair loads fall on odd addresses,
    and n * w * h is no multiple of 4, so the conversion runs its tail - through detect_describe_dev (fp32) and detect_describe_dev_u8
    (8-bit) in two contexts: the region arrays must be the same bytes (geometry, orientation, all 128 descriptor values).  The test
    asserts its own coverage: regions in every size class of the extraction kernels (the three launches of extract_small_kernel, both
    row counts of big_fused_kernel), windows that touch the image border (the checked tap) and windows that do not (the unchecked
    one).  kernels = -1: the library's choice (extract_small_kernel and big_fused_kernel on the 8-bit images); 15: all four, which
    runs the 8-bit form of orient_kernel as well.  big_sample_kernel takes regions with P2 > 1024 only, which images of this size
    cannot hold (the largest window here is 291 pixels wide): here it is launched with an empty work list; given keypoints reach
    it, in both forms, in tests/test_gpu_describe_u8_keys.py."""
    import torch
    w, h = 481, 363
    a, b, _ = synth.pair(w, h, seed=7)
    batch = np.stack([a, b])
    assert np.array_equal(batch, np.round(batch)) and batch.min() >= 0 and batch.max() <= 255
    assert (batch.size % 4) != 0 and (w % 2) == 1
    t32 = torch.from_numpy(batch).cuda()
    t8 = torch.from_numpy(batch.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    c32, c8 = pkg.Context(0, w, h, 2), pkg.Context(0, w, h, 2)
    try:
        c8.set_u8_kernels(kernels)
        nd32, nr32 = c32.detect_describe_dev(t32.data_ptr(), 2, w, h)
        nd8, nr8 = c8.detect_describe_dev_u8(t8.data_ptr(), 2, w, h)
        assert nd32 == nd8 and nr32 == nr8
        assert c8.u8_source_calls() == 1 and c32.u8_source_calls() == 0
        seen = np.zeros(len(P2_CLASSES), np.int64)
        n_touch = n_free = 0
        for i in range(2):
            r32, r8 = c32.regions_fetch(i), c8.regions_fetch(i)
            assert len(r32) == nr32[i] == len(r8) and len(r32) > 100
            for f in r32.dtype.names:
                assert np.array_equal(r32[f], r8[f]), "image %d: field %s differs" % (i, f)
            assert r32.tobytes() == r8.tobytes()
            P2 = _p2(r32)
            seen += np.array([np.count_nonzero((P2 > lo) & (P2 <= hi)) for lo, hi in P2_CLASSES])
            touch, _ = _window_touches(r32, w, h)
            n_touch += np.count_nonzero(touch); n_free += np.count_nonzero(~touch)
        print("regions per P2 class %s, windows touching the border %d, not touching %d" % (seen.tolist(), n_touch, n_free))
        assert (seen > 0).all(), seen
        assert n_touch > 0 and n_free > 0
    finally:
        c32.close(); c8.close()


def test_u8_entry_point_repeated_calls(pkg):
    """The same 8-bit batch three times through one context (the second and third call are repeats: recorded / replayed where the
    scale space forks, eager otherwise), then an fp32 call of the same images: the same regions every time."""
    import torch
    w, h = 320, 240
    a, b, _ = synth.pair(w, h, seed=7)
    batch = np.stack([a, b])
    t32 = torch.from_numpy(batch).cuda()
    t8 = torch.from_numpy(batch.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    try:
        outs = []
        for call in ("u8", "u8", "u8", "f32"):
            if call == "u8":
                ctx.detect_describe_dev_u8(t8.data_ptr(), 2, w, h)
            else:
                ctx.detect_describe_dev(t32.data_ptr(), 2, w, h)
            outs.append([ctx.regions_fetch(i).tobytes() for i in range(2)])
        assert all(o == outs[0] for o in outs[1:]) and len(outs[0][0]) > 0
    finally:
        ctx.close()


def test_fp32_calls_after_u8_call_sample_their_own_images(pkg):
    """An 8-bit call of pair A with every kernel on the 8-bit copies (mask 255: the strip twin is made), then two fp32 calls of ANOTHER
    pair B through the same context - detect_describe_dev of the batch and orient_describe of B's first image with its keys - with A's
    8-bit device tensor overwritten in between.  A call that still sampled from the earlier call's 8-bit images or strips would give
    other regions: both results must be the bytes that a context which never saw an 8-bit image gives, and the counters say that
    one call had the 8-bit sources."""
    import torch
    w, h = 320, 240
    A = np.stack(synth.pair(w, h, seed=7)[:2])
    B = np.stack(synth.pair(w, h, seed=11)[:2])
    assert not np.array_equal(A, B)
    tB = torch.from_numpy(B).cuda()
    t8 = torch.from_numpy(A.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    fresh, ctx = pkg.Context(0, w, h, 2), pkg.Context(0, w, h, 2)
    try:
        fresh.detect_describe_dev(tB.data_ptr(), 2, w, h)
        want_dd = [fresh.regions_fetch(i).tobytes() for i in range(2)]
        keys = fresh.detect_hessian_affine(B[0])
        want_od = fresh.orient_describe(B[0], keys).tobytes()
        assert len(want_dd[0]) > 0 and len(want_dd[1]) > 0 and len(keys) > 100 and len(want_od) > 0
        assert fresh.u8_source_calls() == 0 and fresh.u8_strip_calls() == 0

        ctx.set_u8_kernels(255)
        _, nrA = ctx.detect_describe_dev_u8(t8.data_ptr(), 2, w, h)
        assert min(nrA) > 0 and [ctx.regions_fetch(i).tobytes() for i in range(2)] != want_dd
        t8.zero_()
        torch.cuda.synchronize()
        ctx.detect_describe_dev(tB.data_ptr(), 2, w, h)
        assert [ctx.regions_fetch(i).tobytes() for i in range(2)] == want_dd
        assert ctx.orient_describe(B[0], keys).tobytes() == want_od
        assert ctx.u8_source_calls() == 1 and ctx.u8_strip_calls() == 1
    finally:
        fresh.close(); ctx.close()


RES_FIELDS = ("n_tentatives", "n_unique", "n_inliers", "ransac_samples", "ransac_lo", "ransac_rejects")


def _collect(pipe, n):
    out = []
    for _ in range(n):
        res, tag, m = pipe.next_matches()
        out.append((tag, [getattr(res, f) for f in RES_FIELDS], list(res.n_detected), list(res.n_described), list(res.H), m.copy()))
    return out


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, e in zip(got, want):
        assert g[:5] == e[:5]
        assert np.array_equal(g[5], e[5])


def _pinned_pairs(pkg, w, h, seeds):
    host = [np.stack(synth.pair(w, h, seed=q)[:2]) for q in seeds]
    pin32 = [pkg.PinnedBuffer(x.shape, np.float32) for x in host]
    pin8 = [pkg.PinnedBuffer(x.shape, np.uint8) for x in host]
    for b32, b8, x in zip(pin32, pin8, host):
        b32.array[...] = x
        b8.array[...] = x.astype(np.uint8)
    return pin32, pin8


def _alone_fp32(pkg, pipe, pin32):
    """what each pair gives when it is submitted as fp32 and waited for on its own; no such call has an 8-bit source"""
    pkg.ransac_pin_seed(7)
    before = pipe.u8_source_calls()
    alone = []
    for i, b in enumerate(pin32):
        pipe.submit_host(b.ptr.value, i, u8=False)
        alone += _collect(pipe, 1)
    assert pipe.u8_source_calls() == before
    assert all(a[1][2] > 15 for a in alone)      # verified matches: the pairs are matchable
    return alone


@pytest.fixture(scope="module")
def pipe_pairs(pkg):
    """Two 320 x 240 pairs (w * h * 2 divisible by 4, as 8-bit pairs of a mixed batch must be) in pinned host memory as fp32 and as
    8-bit grey, a pipeline of one GPU worker, one verify worker and two pairs per batch, and the pairs' results from fp32."""
    w, h = 320, 240
    pin32, pin8 = _pinned_pairs(pkg, w, h, (7, 8))
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), 1, 1, 2)
    assert pipe.u8_source_calls() == 1           # the worker's warm-up has loaded the 8-bit forms of the kernels
    alone = _alone_fp32(pkg, pipe, pin32)
    yield pipe, pin32, pin8, alone
    pipe.close()
    for b in pin32 + pin8:
        b.close()


# A GPU worker takes the pairs that are queued when it comes back for work, two at the most: of five pairs submitted back to back the
# first may travel alone, the others follow in batches of two while the worker is busy.  The kinds below make every batch of two
# what the test is about: all 8-bit, or - kinds alternating - one 8-bit and one fp32 pair.  Both paths give the same bits by design,
# so the results cannot tell which one ran: the pipeline's count of calls that had an 8-bit source does.
def test_pipeline_u8_batches_equal_fp32(pkg, pipe_pairs):
    """Batches of 8-bit pairs against the same pairs submitted as fp32: every result field and the verified matches, and every one of
    the three to five batches was described from the staged 8-bit images."""
    pipe, pin32, pin8, alone = pipe_pairs
    pkg.ransac_pin_seed(7)
    before = pipe.u8_source_calls()
    for j in range(5):
        pipe.submit_host(pin8[j % 2].ptr.value, j % 2, u8=True)
    _assert_same(_collect(pipe, 5), [alone[j % 2] for j in range(5)])
    assert 3 <= pipe.u8_source_calls() - before <= 5


def test_pipeline_mixed_batch_falls_back_to_fp32(pkg, pipe_pairs):
    """fp32 and 8-bit pairs alternating, an fp32 pair first, so that a batch of two holds one of each: such a batch has no 8-bit twin,
    both pairs are described from fp32 and give what each gives in a call of its own.  Only an 8-bit pair that happened to travel
    alone (its batch is all 8-bit) may count as a call with an 8-bit source: at most the two 8-bit pairs, none when the five pairs
    travel as 1 + 2 + 2 or 2 + 2 + 1."""
    pipe, pin32, pin8, alone = pipe_pairs
    pkg.ransac_pin_seed(7)
    before = pipe.u8_source_calls()
    for j in range(5):
        if j % 2 == 1:
            pipe.submit_host(pin8[1].ptr.value, 1, u8=True)
        else:
            pipe.submit_host(pin32[0].ptr.value, 0, u8=False)
    _assert_same(_collect(pipe, 5), [alone[j % 2] for j in range(5)])
    n = pipe.u8_source_calls() - before
    print("8-bit pairs of the mixed run that travelled alone: %d" % n)
    assert n <= 2


def test_pipeline_u8_batches_of_odd_size(pkg):
    """481 x 363 pairs: w * h * 2 is no multiple of 4, so the second pair of a batch is staged at an address that is not 4-byte aligned
    and rows start at odd addresses.  A batch of 8-bit pairs is converted in one launch from the (aligned) start of the staging area,
    whatever its size; the results equal those of the fp32 submissions."""
    w, h = 481, 363
    assert (2 * w * h) % 4 != 0
    pin32, pin8 = _pinned_pairs(pkg, w, h, (7, 8))
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), 1, 1, 2)
    try:
        alone = _alone_fp32(pkg, pipe, pin32)
        pkg.ransac_pin_seed(7)
        before = pipe.u8_source_calls()
        for j in range(5):
            pipe.submit_host(pin8[j % 2].ptr.value, j % 2, u8=True)
        _assert_same(_collect(pipe, 5), [alone[j % 2] for j in range(5)])
        assert 3 <= pipe.u8_source_calls() - before <= 5
    finally:
        pipe.close()
        for b in pin32 + pin8:
            b.close()
