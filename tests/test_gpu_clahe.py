"""-m gpu: CLAHE on the MI355X (csrc/clahe.hip) against the numpy restatement tests/clahe_ref.py - single images over sizes, clip
limits, grids and contents, a 32-image 1080p batch, fp32 output with strides, the CLAHE pair pipeline against the plain pipeline
fed equalised images, and the command line's [Matching] doCLAHE against a plain run on equalised PGM files."""
import functools
import os
import subprocess

import numpy as np
import pytest

import clahe_ref
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))

SIZES = [(1920, 1080), (800, 640), (1001, 777), (1000, 777), (37, 29), (9, 7), (5, 3), (1, 1)]
CLIPS = [4.0, 40.0, 1.5, 0.0]
GRIDS = [(8, 8), (4, 6), (1, 1), (16, 9)]
CONTENTS = ["noise", "gradient", "constant", "binary", "graf"]
# 40 of the 640 combinations: every size with every grid and clip limit, every content on every size
CASES = [(SIZES[i], CLIPS[(i + j) % 4], GRIDS[(i + 2 * j + j // 2) % 4], CONTENTS[(i + j) % 5]) for i in range(8) for j in range(5)]


def _rgb(fn):
    from PIL import Image
    return np.asarray(Image.open(fn).convert("RGB"))


@functools.lru_cache(None)
def _graf_u8():
    import orc
    return np.clip(np.rint(orc.grey_of_rgb(_rgb(G1))), 0, 255).astype(np.uint8)     # 800 x 640


def _content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        g = 40 + 120 * xx / max(w - 1, 1) + 60 * yy / max(h - 1, 1) + rng.normal(0, 6, (h, w))
        return np.clip(np.rint(g), 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), 77, np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    g = _graf_u8()
    return np.tile(g, (-(-h // g.shape[0]), -(-w // g.shape[1])))[:h, :w].copy()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0, 1920, 1080, 1)
    yield c
    c.close()


@pytest.mark.parametrize("size,clip,grid,content", CASES)
def test_clahe_matches_restatement(ctx, size, clip, grid, content):
    w, h = size
    img = _content(content, w, h, 1000 * w + h)
    got = ctx.clahe(img, clip, grid)
    assert np.array_equal(got, clahe_ref.clahe(img, clip, grid))


def test_batch_strides_and_fp32(pkg, ctx):
    """32 images of 1080p in one mods_clahe_dev call = 32 single calls; fp32 output = the u8 output as float, with source and
    destination strides above w (aligned and unaligned rows); 8-bit output in place"""
    import torch
    w, h, n = 1920, 1080, 32
    imgs = np.stack([_content(CONTENTS[k % 5], w, h, 100 + k) for k in range(n)])
    src = torch.from_numpy(imgs).cuda()
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    ctx.clahe_dev(src.data_ptr(), n, w, h, dst.data_ptr(), f32=False)
    batch = dst.cpu().numpy()
    for k in range(n):
        assert np.array_equal(batch[k], ctx.clahe(imgs[k])), k
    for k in range(5):
        assert np.array_equal(batch[k], clahe_ref.clahe(imgs[k])), k
    ss = w + 13
    srcp = torch.zeros((n, h, ss), dtype=torch.uint8, device="cuda")
    srcp[:, :, :w] = src
    for ds in (w + 7, w + 64):
        out = torch.full((n, h, ds), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.clahe_dev(srcp.data_ptr(), n, w, h, out.data_ptr(), f32=True, src_stride=ss, dst_stride=ds)
        o = out.cpu().numpy()
        assert np.array_equal(o[:, :, :w], batch.astype(np.float32)), ds
        assert np.all(o[:, :, w:] == -1.0), ds                               # nothing written past the row
    inplace = src.clone()
    torch.cuda.synchronize()
    ctx.clahe_dev(inplace.data_ptr(), n, w, h, inplace.data_ptr(), f32=False)
    assert np.array_equal(inplace.cpu().numpy(), batch)


def _pipeline_run(pkg, stacks, clahe):
    w, h = stacks[0].shape[2], stacks[0].shape[1]
    pinned = []
    for x in stacks:
        buf = pkg.PinnedBuffer(x.shape, np.uint8)
        buf.array[...] = x
        pinned.append(buf)
    pkg.ransac_pin_seed(12345)
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), 4, 8, 16, clahe=clahe)
    got, pending = [], 0
    for i in range(64):
        if pending >= pipe.capacity - 1:
            got.append(pipe.next_matches()); pending -= 1
        pipe.submit_host(pinned[i % len(stacks)].ptr.value, i, u8=True); pending += 1
    while pending:
        got.append(pipe.next_matches()); pending -= 1
    refused = None
    if clahe is not None:     # fp32 pairs are refused by a CLAHE pipeline (OpenCV's CLAHE takes 8-bit images)
        f32 = pkg.PinnedBuffer(stacks[0].shape, np.float32)
        with pytest.raises(pkg.ModsError, match="8-bit"):
            pipe.submit_host(f32.ptr.value, 99)
        with pytest.raises(pkg.ModsError, match="8-bit"):
            pipe.submit(f32.ptr.value, 99)
        f32.close()
        refused = True
    pipe.close()
    for b in pinned:
        b.close()
    return got, refused


def test_pipeline_with_clahe_equals_pipeline_on_equalised_images(pkg):
    """bench.py's pipeline shape (4 GPU workers x 16 pairs, 8 verify workers, pinned 8-bit pairs, seed 12345): CLAHE in the
    pipeline gives what the plain pipeline gives on clahe_ref of the same images - every count, the RANSAC statistics, H, the
    verified matches"""
    import pipeline_oracle as po
    w, h = 1920, 1080
    pairs = po.pmap(lambda i: synth.pair(w, h, seed=2000 + i), range(6), threads=6)
    raw = [np.stack([a, b]).astype(np.uint8) for a, b, _ in pairs]
    eq = po.pmap(lambda r: np.stack([clahe_ref.clahe(x) for x in r]), raw, threads=6)
    got, refused = _pipeline_run(pkg, raw, pkg.ClaheParams.reference())
    want, _ = _pipeline_run(pkg, eq, None)
    assert refused
    assert [t for _, t, _ in got] == [t for _, t, _ in want] == list(range(64))
    for (r, _, m), (q, _, mq) in zip(got, want):
        assert list(r.n_detected) == list(q.n_detected) and list(r.n_described) == list(q.n_described)
        assert (r.n_tentatives, r.n_unique, r.n_inliers) == (q.n_tentatives, q.n_unique, q.n_inliers)
        assert (r.ransac_samples, r.ransac_lo, r.ransac_rejects) == (q.ransac_samples, q.ransac_lo, q.ransac_rejects)
        assert list(r.H) == list(q.H)
        assert np.array_equal(m, mq)
    assert got[0][0].n_inliers > 15


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def _cli(d, img1, img2, load_color, do_clahe):
    d.mkdir()
    text = open(os.path.join(CFG, "classic.ini")).read()
    assert "LoadColor=1;" in text and "[Matching]\n" in text and "doCLAHE" not in text
    text = text.replace("LoadColor=1;", "LoadColor=%d;" % load_color).replace("[Matching]\n", "[Matching]\ndoCLAHE=%d\n" % do_clahe, 1)
    (d / "cfg.ini").write_text(text)
    env = dict(os.environ, MODS_RANSAC_SEED="4242")
    args = [MODS, img1, img2, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(d / "cfg.ini"),
            os.path.join(CFG, "iters_one_view.ini")]
    p = subprocess.run(args, cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    return p.stderr.decode()


def _luma(rgb):
    """imread(..., IMREAD_GRAYSCALE): (R*4899 + G*9617 + B*1868 + 8192) >> 14 (cli/image_io.hpp)"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


@pytest.mark.parametrize("load_color", [1, 0])
def test_cli_do_clahe(pkg, tmp_path, load_color):
    """doCLAHE = 1 on graf1 / graf6 gives the files of a doCLAHE = 0 run on 8-bit PGMs of clahe_ref(rint(grey)) (a PGM feeds the
    pyramid float(v), as the reference's CLAHE branch does), and not those of the plain run"""
    import orc
    grey = (lambda fn: np.clip(np.rint(orc.grey_of_rgb(_rgb(fn))), 0, 255).astype(np.uint8)) if load_color else \
        (lambda fn: _luma(_rgb(fn)))
    p1, p2 = tmp_path / "e1.pgm", tmp_path / "e6.pgm"
    _write_pgm(p1, clahe_ref.clahe(grey(G1)))
    _write_pgm(p2, clahe_ref.clahe(grey(G6)))
    err = _cli(tmp_path / "clahe", G1, G6, load_color, 1)
    assert "CLAHE done in" in err
    _cli(tmp_path / "pgm", str(p1), str(p2), 0, 0)
    _cli(tmp_path / "plain", G1, G6, load_color, 0)
    a, b, c = tmp_path / "clahe", tmp_path / "pgm", tmp_path / "plain"
    for fn in ("m.txt", "k1.txt", "k2.txt", "H.txt"):
        assert (a / fn).read_text() == (b / fn).read_text(), fn
    la, lb = (a / "log.txt").read_text().split(), (b / "log.txt").read_text().split()
    assert len(la) == len(lb) == 7 and la[1:] == lb[1:]                   # every field but the time
    assert int(la[1]) > 15
    assert (a / "k1.txt").read_text() != (c / "k1.txt").read_text()      # the key is not ignored
    assert (a / "m.txt").read_text() != (c / "m.txt").read_text()
