"""CPU tests of the detection masks: the host statement of the on-mask rule (mods_detection_mask_test) against the numpy rule of
tests/detection_mask_ref.py, and the command line's handling of a missing or mis-sized [DetectionMask] file (reported before a
device is looked for)."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import detection_mask_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))


def write_png_grey(fn, a):
    """an 8-bit grey PNG of the 2-D uint8 array a"""
    a = np.ascontiguousarray(a, np.uint8)
    h, w = a.shape
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(fn, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) +
                chunk(b"IEND", b""))


def _ulp_neighbours(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def _edge_points(w, h):
    """coordinates where the rounding decides: k +- 0.5 and one ulp to either side, for pixels at the borders and inside; negative
    coordinates; x = w - 0.5; far outside; non-finite"""
    xs = []
    for k in (0, 1, 2, 7, w - 2, w - 1, w):
        for d in (-0.5, 0.5):
            xs += _ulp_neighbours(np.float64(k) + d)
    xs += [-0.5 - 1e-9, -1.0, -3.25, -1e30, 1e30, float(w) - 0.5, float(w), np.nan, np.inf, -np.inf, 0.49999999999999994, 4.0e9]
    ys = []
    for k in (0, 1, 5, h - 1, h):
        for d in (-0.5, 0.5):
            ys += _ulp_neighbours(np.float64(k) + d)
    ys += [-0.75, -2.0, float(h) - 0.5, np.nan, 3.0e9]
    return np.array(xs, np.float64), np.array(ys, np.float64)


@pytest.mark.parametrize("w,h", [(9, 7), (33, 5)])
def test_rule_matches_numpy_at_the_rounding_edges(pkg, w, h):
    rng = np.random.default_rng(w * 100 + h)
    mask = np.where(rng.uniform(size=(h, w)) < 0.5, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)
    assert (mask == 0).sum() >= 5 and (mask != 0).sum() >= 5
    xs, ys = _edge_points(w, h)
    gx, gy = np.meshgrid(xs, ys)
    want = ref.on_mask(mask, gx.ravel(), gy.ravel())
    got = np.array([pkg.detection_mask_test(mask, x, y) for x, y in zip(gx.ravel(), gy.ravel())])
    assert np.array_equal(got, want)
    assert want.sum() >= 5 and (~want).sum() >= 5
    # spot checks of the rule as the header states it, without the reference: pixel centres sit at integer coordinates
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = 1
    assert pkg.detection_mask_test(m, -0.5, -0.5) and pkg.detection_mask_test(m, 0.49, 0.49)
    assert not pkg.detection_mask_test(m, 0.5, 0.0) and not pkg.detection_mask_test(m, np.nextafter(-0.5, -np.inf), 0.0)
    m[:] = 0
    m[h - 1, w - 1] = 200
    assert pkg.detection_mask_test(m, w - 1.5, h - 1.5) and pkg.detection_mask_test(m, np.nextafter(w - 0.5, 0), h - 1)
    assert not pkg.detection_mask_test(m, w - 0.5, h - 1) and not pkg.detection_mask_test(m, w - 1, h - 0.5)


def test_rule_reads_rows_by_their_stride(pkg):
    """stride > w: the padding bytes are poison of the opposite kind and must never decide"""
    w, h = 11, 6
    rng = np.random.default_rng(5)
    dense = np.where(rng.uniform(size=(h, w)) < 0.5, 0, 255).astype(np.uint8)
    for poison in (255, 0):
        padded = ref.with_row_padding(dense, pad=13, poison=poison)
        assert padded.strides[0] == w + 13
        xs, ys = _edge_points(w, h)
        gx, gy = np.meshgrid(xs, ys)
        want = ref.on_mask(dense, gx.ravel(), gy.ravel())
        got = np.array([pkg.detection_mask_test(padded, x, y) for x, y in zip(gx.ravel(), gy.ravel())])
        assert np.array_equal(got, want)
    # the C entry point refuses what is no mask: 0, not a crash
    L = pkg.lib()
    import ctypes as C
    assert L.mods_detection_mask_test(None, 4, 4, 4, C.c_double(1), C.c_double(1)) == 0
    buf = (C.c_ubyte * 16)(*([1] * 16))
    assert L.mods_detection_mask_test(buf, 4, 4, 3, C.c_double(1), C.c_double(1)) == 0      # stride < w
    assert L.mods_detection_mask_test(buf, 4, 4, 4, C.c_double(1), C.c_double(1)) == 1


def test_filter_regions_keeps_order():
    regs = np.zeros(6, [("x", "f8"), ("y", "f8"), ("id", "i4")])
    regs["x"] = [0.2, 3.6, 1.0, -0.6, 2.5, 2.49]
    regs["y"] = 0.0
    regs["id"] = np.arange(6)
    mask = np.array([[1, 0, 1, 0]], np.uint8)
    assert list(ref.filter_regions(regs, mask)["id"]) == [0, 5]       # 3.6 -> 4 (outside), 2.5 -> 3 (off), 2.49 -> 2 (on)


def _cli(tmp_path, ini_tail, img1=G1):
    text = open(os.path.join(CFG, "classic.ini")).read() + "\n" + ini_tail + "\n"
    (tmp_path / "mask.ini").write_text(text)
    p = subprocess.run([MODS, img1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp_path / "mask.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stderr.decode()


def test_cli_reports_missing_and_mis_sized_mask_files(pkg, tmp_path):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    rc, err = _cli(tmp_path, "[DetectionMask]\nmask1 = no_such_mask.png")
    assert rc == 1 and "Cannot read detection mask no_such_mask.png" in err and "mask1" in err
    write_png_grey(tmp_path / "small.png", np.full((64, 80), 255, np.uint8))
    rc, err = _cli(tmp_path, "[DetectionMask]\nmask2 = small.png")
    assert rc == 1 and "Detection mask small.png is 80x64, image 2 is 800x640" in err
    assert not os.path.exists(tmp_path / "m.txt")
    # useMaskFiles = 1: <image path without extension>_mask.png is looked for, found, and checked like a named one
    shutil.copy(G1, tmp_path / "first.png")
    write_png_grey(tmp_path / "first_mask.png", np.full((10, 10), 255, np.uint8))
    rc, err = _cli(tmp_path, "[DetectionMask]\nuseMaskFiles = 1", img1=str(tmp_path / "first.png"))
    assert rc == 1 and "first_mask.png is 10x10, image 1 is 800x640" in err
