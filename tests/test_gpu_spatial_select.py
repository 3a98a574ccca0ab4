"""-m gpu: the spatial selection of the count modes' cut (mods_ctx_spatial_selection, csrc/spatial_select.hip).  Every expected
value is tests/spatial_select_ref.py's, bit for bit: the test hook's indices on constructed lists, and the keys, regions and
matches of the entry points that detect, against the restatement applied to the list the same call returns with the selection
off and the count unrestricted."""
import math
import os
import subprocess

import numpy as np
import pytest

import spatial_select_ref as ref
import synth
from detection_mask_ref import assert_same_but_positions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
W, H = 256, 192
KEY_FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "octave", "level", "r0", "c0")
CS = (1.0, 0.9, 0.0)
ALL = 10 ** 6                                  # a regionsNumber no list reaches: the count modes' list uncut
_radii = {}                                    # (list name, c) -> r2: a list's radii are computed once for all its keep values


def _keys(pkg, xyr):
    x, y, r = xyr
    k = np.zeros(len(r), pkg.AFFKEY_DTYPE)
    k["x"], k["y"], k["response"] = x, y, r
    k["s"], k["a11"], k["a22"] = 2.0, 1.0, 1.0
    k["c0"] = np.arange(len(r))                # (no two keys of a list are the same bytes)
    return k


def _want(name, xyr, keep, c):
    if (name, c) not in _radii:
        _radii[(name, c)] = ref.radii(*xyr, c)
    return ref.pick(_radii[(name, c)], keep).tolist()


def _keeps(n):
    return [0, 1, n - 1, n, n + 7, n // 3]


def _check_hook(pkg, ctx, slots, c):
    """slots: (name, xyr, keep) per image slot of one call"""
    got = ctx.test_spatial_select([_keys(pkg, xyr) for _, xyr, _ in slots], [keep for _, _, keep in slots], c)
    for g, (name, xyr, keep) in zip(got, slots):
        assert g.tolist() == _want(name, xyr, keep, c), (name, len(xyr[2]), keep, c)


@pytest.fixture(scope="module")
def hctx(pkg):
    """six image slots of 65 536 keys"""
    ctx = pkg.Context(0, 64, 64, 6)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_hook_on_random_lists(pkg, hctx, n):
    """wave edges and the edges of the 1024-key LDS tiles; the six keep values as six images of one call (ranked by the sort), then
    as two calls of three (ranked by counting)"""
    xyr = ref.random_list(n, seed=100 + n)
    slots = [("random%d" % n, xyr, keep) for keep in _keeps(n)]
    for c in CS:
        _check_hook(pkg, hctx, slots, c)
        _check_hook(pkg, hctx, slots[:3], c)
        _check_hook(pkg, hctx, slots[3:], c)


def test_hook_at_the_rank_sort_limit(pkg, hctx):
    """16 384 keys are the most one workgroup sorts, 16 385 fall back to counting inside a call of five images"""
    lists = [("random%d" % n, ref.random_list(n, seed=100 + n)) for n in (16384, 16385)]
    combos = [(name, xyr, _keeps(len(xyr[2]))[i]) for i in range(6) for name, xyr in lists]
    for c in CS:
        for at in range(0, len(combos), 5):
            slots = (combos[at:at + 5] + combos[:5])[:5]
            assert len(slots) == 5
            _check_hook(pkg, hctx, slots, c)


def test_hook_on_one_image_ranked_by_counting(pkg, hctx):
    xyr = ref.random_list(3000, seed=3100)
    for c in CS:
        for keep in _keeps(3000):
            _check_hook(pkg, hctx, [("random3000", xyr, keep)], c)


@pytest.mark.parametrize("name", ["lattice", "tied_response", "duplicate_position", "equal_radius"])
def test_hook_on_lists_built_to_tie(pkg, hctx, name):
    """equal radii everywhere: the smaller index decides (the constructions are held to their purpose in test_cpu_spatial_select)"""
    xyr = getattr(ref, name + "_list")()
    n = len(xyr[2])
    for c in ((0.9,) if name == "equal_radius" else (1.0, 0.9)):
        for keep in (n // 3, n // 2, n - 1, 2):
            _check_hook(pkg, hctx, [(name, xyr, keep)], c)                                   # counting
        _check_hook(pkg, hctx, [(name, xyr, keep) for keep in (n // 3, n // 2, n - 1, 2, n // 5)], c)   # the sort
    if name == "equal_radius":
        assert hctx.test_spatial_select([_keys(pkg, xyr)], [40], 0.9)[0].tolist() == list(range(40))


@pytest.mark.parametrize("n_img", [4, 5])
def test_hook_on_lists_of_unequal_length(pkg, hctx, n_img):
    """an empty list and a list of one key between long ones: each image's own base offset, count and keep"""
    sizes = [2049, 0, 1, 1500, 700][:n_img]
    keeps = [700, 3, 1, 500, 233][:n_img]
    slots = [("random%d" % n, ref.random_list(n, seed=100 + n) if n else tuple(np.zeros(0, np.float32) for _ in range(3)), keep)
             for n, keep in zip(sizes, keeps)]
    for c in (1.0, 0.9):
        _check_hook(pkg, hctx, slots, c)
    got = hctx.test_spatial_select([_keys(pkg, s[1]) for s in slots], keeps, 0.9)
    assert [len(g) for g in got] == [700, 0, 1, 500, 233][:n_img]


def test_clustered_scene(pkg, hctx):
    """300 strong keys in a 10 x 10 px square, 100 weaker ones spread on a 50 px lattice, 100 to keep: the cut by response keeps
    the square alone, the selection keeps its strongest key and 99 of the lattice.  Fails without the feature."""
    xyr = ref.clustered_scene()
    for n_img in (1, 5):
        got = hctx.test_spatial_select([_keys(pkg, xyr)] * n_img, [100] * n_img, 1.0)
        for g in got:
            assert g.tolist() == ref.select(*xyr, 100, 1.0).tolist()
            assert len(g) == 100 and g[0] == 0 and np.count_nonzero(g >= 300) == 99
    assert np.count_nonzero(np.arange(100) >= 300) == 0


# ---- through the detector
def _det(pkg, det, **over):
    p = {"hessian": pkg.HessAffParams.default, "dog": pkg.HessAffParams.dog, "harris": pkg.HessAffParams.harris}[det]()
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _same_keys(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in KEY_FIELDS:
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8)), f


def _regions_of(regs, keys_all, sel):
    """the regions of the list `regs` (described from keys_all) whose key is in sel: the response names the key"""
    assert len(np.unique(keys_all["response"])) == len(keys_all)
    return regs[np.isin(regs["response"], sel["response"])]


@pytest.fixture(scope="module")
def batch6():
    import torch
    imgs = np.stack([synth.texture(W, H, seed=20 + i) for i in range(6)])
    t = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    return imgs, t


@pytest.fixture(scope="module")
def ctx6(pkg):
    ctx = pkg.Context(0, W, H, 6)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("det", ["hessian", "dog", "harris"])
def test_end_to_end_keys(pkg, ctx6, batch6, det):
    """mods_detect_hessian_affine_dev on one image and on six: FixedRegNumber at a third of the uncut count, RelativeRegNumber 0.5"""
    _, t = batch6
    ctx6.spatial_selection(0)
    for n_img in (1, 6):
        every = ctx6.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, _det(pkg, det, mode=2, regionsNumber=ALL))
        third = len(every[0]) // 3
        assert third >= 30 and all(np.all(np.diff(np.abs(k["response"])) <= 0) for k in every)
        for c in (0.9, 1.0):
            ctx6.spatial_selection(1, c)
            assert ctx6.spatial_selection_get() == (1, c)
            fixed = ctx6.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, _det(pkg, det, mode=2, regionsNumber=third))
            rel = ctx6.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, _det(pkg, det, mode=3, relativeRegionsNumber=0.5))
            uncut = ctx6.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, _det(pkg, det, mode=2, regionsNumber=ALL))
            ctx6.spatial_selection(0)
            for i in range(n_img):
                want = ref.select_keys(every[i], ref.keep_count(2, len(every[i]), third), c)
                _same_keys(fixed[i], want)
                assert len(fixed[i]) == min(third, len(every[i]))
                if len(every[i]) > third:
                    assert not np.array_equal(want["response"], every[i]["response"][:third])      # (not the prefix)
                _same_keys(rel[i], ref.select_keys(every[i], ref.keep_count(3, len(every[i]), relative_regions_number=0.5), c))
                _same_keys(uncut[i], every[i])
        # off after having been on: the cut by response again
        again = ctx6.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, _det(pkg, det, mode=2, regionsNumber=third))
        for i in range(n_img):
            _same_keys(again[i], every[i][:third])


def test_described_regions_are_the_selected_keys(pkg, ctx6, batch6):
    """mods_detect_describe_dev: orientation and description see the selected list"""
    imgs, t = batch6
    ctx6.spatial_selection(0)
    every = ctx6.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, _det(pkg, "hessian", mode=2, regionsNumber=ALL))
    ctx6.detect_describe_dev(t.data_ptr(), 2, W, H, det=_det(pkg, "hessian", mode=2, regionsNumber=ALL))
    regs_every = [ctx6.regions_fetch(i) for i in range(2)]
    ctx6.spatial_selection(1, 0.9)
    try:
        nd, nr = ctx6.detect_describe_dev(t.data_ptr(), 2, W, H, det=_det(pkg, "hessian", mode=2, regionsNumber=60))
        got = [ctx6.regions_fetch(i) for i in range(2)]
    finally:
        ctx6.spatial_selection(0)
    assert nd == [60, 60]
    for i in range(2):
        sel = ref.select_keys(every[i], 60, 0.9)
        want = _regions_of(regs_every[i], every[i], sel)
        assert nr[i] == len(want) > 30
        assert_same_but_positions(got[i], want)
        assert_same_but_positions(got[i], ctx6.orient_describe(imgs[i], sel))


def test_view_keeps_its_scaled_count(pkg):
    """mods_detect_describe_view_dev at tilt 3: the view keeps floor(regionsNumber / 3) keys, chosen in the view's frame"""
    import torch
    w, h, tilt, phi, number = 320, 240, 3.0, math.pi / 3, 240
    img = synth.texture(w, h, seed=3)
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    try:
        t = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        g, nd_all, _ = ctx.detect_describe_view_dev(t.data_ptr(), w, h, tilt, phi, det=_det(pkg, "hessian", mode=2, regionsNumber=ALL))
        regs_all = ctx.regions_fetch(0)
        keys_all = ctx.detect_hessian_affine(ctx.view_pixels(g), _det(pkg, "hessian", mode=2, regionsNumber=ALL))
        keep = int(math.floor(1.0 * number / tilt))
        assert len(keys_all) == nd_all > 2 * keep
        sel = ref.select_keys(keys_all, keep, 0.9)
        ctx.spatial_selection(1, 0.9)
        _, nd, nr = ctx.detect_describe_view_dev(t.data_ptr(), w, h, tilt, phi, det=_det(pkg, "hessian", mode=2, regionsNumber=number))
        got = ctx.regions_fetch(0)
        want = _regions_of(regs_all, keys_all, sel)
        assert nd == keep and nr == len(got) == len(want) >= 20           # (most of a tilted view's keys fall outside the image)
        assert_same_but_positions(got, want)
        assert not np.array_equal(np.sort(sel["response"]), np.sort(keys_all["response"][:keep]))
    finally:
        ctx.close()


def test_recorded_graphs(pkg):
    """mods_ctx_graphs on a batch whose scale space forks (the calls that are recorded): the replays return the eager calls'
    regions, and a change of the robustness is not served from the recording of the other value"""
    import torch
    w, h = 2048, 1024
    img = np.tile(synth.texture(512, 256, seed=4), (4, 4))
    t = torch.from_numpy(np.stack([img, img[::-1].copy()])).cuda()
    torch.cuda.synchronize()
    par = _det(pkg, "hessian", mode=2, regionsNumber=2000)
    ctx = pkg.Context(0, w, h, 2)
    try:
        def call():
            nd, _ = ctx.detect_describe_dev(t.data_ptr(), 2, w, h, det=par)
            assert nd == [2000, 2000]
            return [ctx.regions_fetch(i).tobytes() for i in range(2)]
        call()                                                  # (the call that sizes the context's pools is never a repeat)
        plain = call()
        ctx.spatial_selection(1, 0.9)
        want_a = call()
        ctx.spatial_selection(1, 0.5)
        want_b = call()
        assert want_a != want_b and want_a != plain and ctx.graph_replays() == 0
        ctx.graphs(True)
        ctx.spatial_selection(1, 0.9)
        assert [call() for _ in range(3)] == [want_a] * 3
        assert ctx.graph_replays() >= 1
        ctx.spatial_selection(1, 0.5)
        assert [call() for _ in range(2)] == [want_b] * 2
        ctx.spatial_selection(0)
        assert [call() for _ in range(2)] == [plain] * 2
    finally:
        ctx.close()


def test_the_selection_adds_no_launch_when_off(pkg, ctx6, batch6):
    _, t = batch6
    par = _det(pkg, "hessian", mode=2, regionsNumber=50)
    ctx6.spatial_selection(0)
    ctx6.timing_enable(["sort", "spatial_select"])
    try:
        ctx6.timing_reset()
        ctx6.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par, fetch=False)
        assert ctx6.timing_read("spatial_select")[1] == 0 and ctx6.timing_read("sort")[1] == 1
        ctx6.spatial_selection(1, 0.9)
        ctx6.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par, fetch=False)
        assert ctx6.timing_read("spatial_select")[1] == 1 and ctx6.timing_read("sort")[1] == 2
    finally:
        ctx6.spatial_selection(0)
        ctx6.timing_enable([])


def test_refusals(pkg, ctx6, batch6):
    _, t = batch6
    ctx6.spatial_selection(1, 0.9)
    try:
        for mode, word in ((0, "mode = FixedTh"), (1, "mode = RelativeTh"), (4, "mode = NotLessThanRegions")):
            with pytest.raises(pkg.ModsError, match="spatial_selection: " + word):
                ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=mode, relativeThreshold=0.1, regionsNumber=50))
        with pytest.raises(pkg.ModsError, match="spatial_selection: detectorType = MSER"):
            ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, pkg.HessAffParams.mser(mode=2, reg_number=50))
        with pytest.raises(pkg.ModsError, match="spatial_selection: mode = FixedTh"):
            ctx6.detect_describe_dev(t.data_ptr(), 1, W, H)
        for c in (1.5, -0.01, float("nan")):
            with pytest.raises(pkg.ModsError, match="spatial_selection: robustness"):
                ctx6.spatial_selection(1, c)
        with pytest.raises(pkg.ModsError, match="spatial_selection: mode 3"):
            ctx6.spatial_selection(3, 0.9)
        assert ctx6.spatial_selection_get() == (1, 0.9)                 # a refused setting changes nothing
        # mode 2: the calls the selection does not cover run as they do without it
        ctx6.spatial_selection(0)
        plain = ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H)[0]
        mser = ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, pkg.HessAffParams.mser(mode=2, reg_number=50))[0]
        ctx6.spatial_selection(2, 0.9)
        _same_keys(ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H)[0], plain)
        _same_keys(ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, pkg.HessAffParams.mser(mode=2, reg_number=50))[0], mser)
        every = ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=2, regionsNumber=ALL))[0]
        _same_keys(ctx6.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=2, regionsNumber=50))[0],
                   ref.select_keys(every, 50, 0.9))
    finally:
        ctx6.spatial_selection(0)


def _pair_params(pkg, number):
    par = pkg.PairParams.default()
    par.det.mode, par.det.regionsNumber = 2, number
    return par


def test_pair_and_pipeline(pkg):
    """mods_match_pair_dev keeps the selected keys of both images; the pipeline with mods_pipeline_spatial_selection returns what
    mods_match_pair_dev returns on a context set the same way"""
    import torch
    w, h, number = 320, 240, 150
    pairs = [synth.pair(w, h, seed=s)[:2] for s in (0, 5, 9)]
    par = _pair_params(pkg, number)
    ctx = pkg.Context(0, w, h, 2)
    pipe = pkg.Pipeline(0, w, h, params=par, gpu_workers=1, verify_workers=1, pairs_per_batch=2)
    try:
        want = []
        for a, b in pairs:
            t = torch.from_numpy(np.stack([a, b])).cuda()
            torch.cuda.synchronize()
            ctx.spatial_selection(0)
            every = ctx.detect_hessian_affine_dev(t.data_ptr(), 2, w, h, _det(pkg, "hessian", mode=2, regionsNumber=ALL))
            ctx.detect_describe_dev(t.data_ptr(), 2, w, h, det=_det(pkg, "hessian", mode=2, regionsNumber=ALL))
            regs_every = [ctx.regions_fetch(i) for i in range(2)]
            pkg.ransac_pin_seed(11)
            plain, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par, max_matches=10000)
            ctx.spatial_selection(1, 0.9)
            pkg.ransac_pin_seed(11)
            res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par, max_matches=10000)
            regs = [ctx.regions_fetch(i) for i in range(2)]
            for i in range(2):
                assert_same_but_positions(regs[i], _regions_of(regs_every[i], every[i], ref.select_keys(every[i], number, 0.9)))
            assert list(res.n_detected) == [number, number] == list(plain.n_detected)
            want.append((res, m))
        pipe.spatial_selection(1, 0.9)
        pkg.ransac_pin_seed(11)
        u8 = [pkg.PinnedBuffer((2, h, w), np.uint8) for _ in pairs]
        for k, (a, b) in enumerate(pairs):
            u8[k].array[:] = np.stack([a, b]).astype(np.uint8)
            pipe.submit_host(u8[k].ptr.value, tag=k, u8=True)
        for k in range(len(pairs)):
            res, tag, m = pipe.next_matches()
            exp, exp_m = want[k]
            assert tag == k
            for f in ("n_tentatives", "n_unique", "n_inliers"):
                assert getattr(res, f) == getattr(exp, f), (tag, f)
            assert list(res.n_detected) == list(exp.n_detected) and list(res.n_described) == list(exp.n_described)
            assert np.array_equal(m, exp_m) and list(res.H) == list(exp.H), tag
        with pytest.raises(pkg.ModsError, match="after the first submit"):
            pipe.spatial_selection(0)
        for b in u8:
            b.close()
    finally:
        pkg.ransac_pin_seed(-1)
        pipe.close(); ctx.close()


# ---- the command line
def _cli(tmp_path, name, section, img1, img2, number):
    text = open(os.path.join(CFG, "classic.ini")).read()
    assert "[HessianAffine]\nmode=FixedTh;" in text
    text = text.replace("[HessianAffine]\nmode=FixedTh;", "[HessianAffine]\nmode=FixedRegNumber;\nregionsNumber = %d;" % number, 1)
    (tmp_path / "c.ini").write_text(text + "\n" + section + "\n")
    out = tmp_path / name
    out.mkdir()
    p = subprocess.run([MODS, img1, img2, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=out, env=dict(os.environ, MODS_RANSAC_SEED="4242"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return {fn: (out / fn).read_bytes() for fn in ("k1.txt", "k2.txt", "m.txt")}, p.stderr.decode()


def test_cli(pkg, tmp_path):
    """[SpatialSelection] on a FixedRegNumber step of a 320 x 240 pair.  The keypoint files list the regions that were described:
    regionsNumber keys are selected (checked through the library), the ones orientation and description keep have a row each, and
    those rows are the library's regions.  Without the section, and with doSpatialSelection = 0, the files are those of the
    library with the selection off."""
    import torch
    from test_cpu_detection_mask import write_png_grey
    w, h, number = 320, 240, 120
    a, b, _ = synth.pair(w, h)
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    f1, f2 = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    write_png_grey(f1, a)
    write_png_grey(f2, b)
    on, err = _cli(tmp_path, "on", "[SpatialSelection]\ndoSpatialSelection = 1\nrobustness = 0.9", f1, f2, number)
    absent, _ = _cli(tmp_path, "absent", "", f1, f2, number)
    off, _ = _cli(tmp_path, "off", "[SpatialSelection]\ndoSpatialSelection = 0", f1, f2, number)
    assert absent == off and on["k1.txt"] != absent["k1.txt"] and on["k2.txt"] != absent["k2.txt"]
    assert "Spatial selection (ANMS): robustness 0.9" in err and "Note: [SpatialSelection]" not in err

    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep = [pkg.ImgRep(ctx) for _ in range(4)]
    try:
        t = torch.from_numpy(np.stack([a, b]).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        par = _pair_params(pkg, number)
        steps = [pkg.LadderStep.make((1,), 360.0)]
        every, regs_every = [], []
        for i in range(2):
            every += ctx.detect_hessian_affine_dev(t.data_ptr() + 4 * i * w * h, 1, w, h, _det(pkg, "hessian", mode=2, regionsNumber=ALL))
            ctx.detect_describe_dev(t.data_ptr() + 4 * i * w * h, 1, w, h, det=_det(pkg, "hessian", mode=2, regionsNumber=ALL))
            regs_every.append(ctx.regions_fetch(0))
        pkg.ransac_pin_seed(4242)
        pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep[0], rep[1], par, max_matches=1 << 16)
        ctx.spatial_selection(1, 0.9)
        pkg.ransac_pin_seed(4242)
        res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep[2], rep[3], par, max_matches=1 << 16)
        assert list(res.n_detected) == [number, number]
        for i in range(2):      # the ladder's banks are the selected keys' regions
            assert_same_but_positions(rep[2 + i].fetch(), _regions_of(regs_every[i], every[i], ref.select_keys(every[i], number, 0.9)))
        for files, banks in ((absent, rep[:2]), (on, rep[2:])):
            for fn, bank in zip(("k1.txt", "k2.txt"), banks):
                r = bank.fetch()
                lines = files[fn].decode().splitlines()
                assert lines[2] == "RootSIFT %d" % len(r) and len(lines) == 4 + len(r) and number // 2 < len(r) <= number
                rows = np.array([ln.split() for ln in lines[4:]], float)
                want = np.stack([r[f] for f in ("x", "y", "s", "a11", "a12", "a21", "a22")], axis=1)
                assert np.allclose(rows[:, :7], want, rtol=1e-5) and np.array_equal(rows[:, 8:], r["desc"].astype(float))
        got = np.loadtxt(tmp_path / "on" / "m.txt", ndmin=2)
        assert len(got) == res.n_inliers and (len(got) == 0 or np.allclose(got, m, rtol=1e-5, atol=1e-3))
    finally:
        pkg.ransac_pin_seed(-1)
        for r in rep:
            r.close()
        ctx.close()


def test_cli_notes(pkg, tmp_path):
    """a FixedTh step runs as before under the section, with one Note under verbose"""
    from test_cpu_detection_mask import write_png_grey
    w, h = 320, 240
    a, b, _ = synth.pair(w, h)
    f1, f2 = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    write_png_grey(f1, a.astype(np.uint8))
    write_png_grey(f2, b.astype(np.uint8))

    def run(name, section):
        (tmp_path / (name + ".ini")).write_text(open(os.path.join(CFG, "classic.ini")).read() + "\n" + section + "\n")
        out = tmp_path / name
        out.mkdir()
        p = subprocess.run([MODS, f1, f2, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp_path / (name + ".ini")),
                            os.path.join(CFG, "iters_one_view.ini")], cwd=out, env=dict(os.environ, MODS_RANSAC_SEED="4242"),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return {fn: (out / fn).read_bytes() for fn in ("k1.txt", "k2.txt", "m.txt")}, p.stderr.decode()
    plain, _ = run("plain", "")
    noted, err = run("noted", "[SpatialSelection]\ndoSpatialSelection = 1")
    assert noted == plain and err.count("Note: [SpatialSelection]") == 1 and "run as before: HessianAffine" in err
