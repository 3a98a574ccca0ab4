"""The strip layout of the 8-bit images the samplers gather from (csrc/u8_strips.hpp), through the library's host-only export of that
header: strips of 15 columns stored as 16 bytes per image row - a strip's own columns and the first one of the next strip - rows
consecutive, a strip's rows padded to a multiple of 8.  No GPU."""
import numpy as np
import pytest

WIDTHS = (16, 17, 31, 481, 1920)
HEIGHTS = (9, 16, 363)


def strips_of(img, pkg):
    """the layout restated in numpy: [n_strips][h8][16], zero where the layout pads"""
    h, w = img.shape
    _, ns, pitch, nbytes = pkg.u8_strips_layout(w, h)
    h8 = -(-h // 8) * 8
    assert ns == -(-(w - 1) // 15) and pitch == 16 * h8 and nbytes == ns * pitch
    out = np.zeros((ns, h8, 16), np.uint8)
    for s in range(ns):
        cols = img[:, 15 * s:15 * s + 16]
        out[s, :h, :cols.shape[1]] = cols
    return out


def test_multiply_shift_is_division_by_15(pkg):
    """(x * 0x8889) >> 19 == x // 15 for every x below the limit the library asserts where it makes the strips - and the limit is the
    first x at which it fails, so no image the library accepts is wider than what the arithmetic covers"""
    limit = pkg.u8_strips_layout(16, 9)[0]
    assert limit > 1920
    got = pkg.u8_strips_strip_of(limit + 1)
    x = np.arange(limit + 1, dtype=np.int64)
    assert np.array_equal(got[:limit], x[:limit] // 15)
    assert np.array_equal(got, (x * 0x8889) >> 19)
    assert got[limit] != limit // 15
    with pytest.raises(pkg.ModsError, match="outside the layout"):
        pkg.u8_strips_layout(limit, 16)
    assert pkg.u8_strips_layout(limit - 1, 16)[1] == -(-(limit - 2) // 15)


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_pair_maps_inside_the_buffer(pkg, w, h):
    """every (x <= w - 2, y <= h - 2): the pair's two bytes, and those of the row below (+ 16), lie inside the image's strips, in one
    16-byte row each, and no two pixels outside the shared columns map to one byte"""
    _, ns, pitch, nbytes = pkg.u8_strips_layout(w, h)
    off = pkg.u8_strips_offsets(w, h).astype(np.int64)
    assert off.shape == (h - 1, w - 1)
    assert off.min() >= 0 and (off + 16 + 1).max() < nbytes
    assert ((off % 16) <= 14).all()                                  # x and x + 1 in the same 16-byte row
    x = np.arange(w - 1)[None, :]
    y = np.arange(h - 1)[:, None]
    assert np.array_equal(off, (x // 15) * pitch + 16 * y + x % 15)
    assert len(np.unique(off)) == off.size


@pytest.mark.parametrize("w,h", [(16, 9), (17, 16), (31, 9), (481, 363), (250, 170), (1920, 16)])
def test_pairs_read_through_the_offsets_are_the_row_major_pixels(pkg, w, h):
    """a random image laid out in numpy: the four pixels of every tap - (x, y), (x + 1, y) at the offset and the next byte,
    (x, y + 1), (x + 1, y + 1) 16 bytes on - are the row-major image's"""
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    flat = strips_of(img, pkg).reshape(-1)
    off = pkg.u8_strips_offsets(w, h).astype(np.int64)
    assert np.array_equal(flat[off], img[:-1, :-1])
    assert np.array_equal(flat[off + 1], img[:-1, 1:])
    assert np.array_equal(flat[off + 16], img[1:, :-1])
    assert np.array_equal(flat[off + 17], img[1:, 1:])
