"""The contract of the doubled first octave (mods_ctx_upscale_input) as tests/upscale_ref.py restates it, checked on the CPU:
double_image by hand, its summation order, its last row and column, the composed scale space against the oracle where both skip
the initial blur, and the library's exports.  Every comparison is np.array_equal."""
import functools

import numpy as np
import pytest

import orc
import synth
import upscale_ref as ur


def _f32(rows):
    return np.array(rows, np.float32)


def test_double_image_by_hand():
    assert np.array_equal(ur.double_image(_f32([[3.0]])), _f32([[3, 3], [3, 3]]))
    row = _f32([[1, 2, 4, 8, 16, 32, 64]])
    want = _f32([1, 1.5, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 64])
    assert np.array_equal(ur.double_image(row), np.stack([want, want]))
    assert np.array_equal(ur.double_image(row.T), np.stack([want, want]).T)
    assert np.array_equal(ur.double_image(_f32([[0, 2], [4, 8]])),
                          _f32([[0, 1, 2, 2],
                                [2, 3.5, 5, 5],
                                [4, 6, 8, 8],
                                [4, 6, 8, 8]]))


def test_double_image_sums_in_the_contracts_order():
    """a, b, c_, d = 1e8, 1, -1e8, 1: ((a + b) + c_) + d = ((1e8) - 1e8) + 1 = 1 in fp32 (1e8 + 1 = 1e8), so the centre is 0.25; any
    other association of the four gives 0.5 or 0."""
    d = ur.double_image(_f32([[1e8, 1], [-1e8, 1]]))
    assert d[1, 1] == np.float32(0.25)
    assert d[0, 1] == np.float32(0.5) * (np.float32(1e8) + np.float32(1)) and d[1, 0] == np.float32(0)


@pytest.mark.parametrize("w,h", [(7, 5), (8, 6), (1, 4), (5, 1)])
def test_last_odd_row_and_column_repeat_their_even_neighbours(w, h):
    """r' = r and c' = c at the last row and column.  On 8-bit valued pixels (every sum below is exact) the whole last odd row and
    column equal row 2h - 2 and column 2w - 2; on any pixels their even-indexed entries do (0.5f * (a + a) = a), while an odd-odd
    entry is 0.25f * (((a + b) + a) + b), which rounds twice where its neighbour 0.5f * (a + b) rounds once: the formula is the
    contract there."""
    rng = np.random.default_rng(5)
    img8 = rng.integers(0, 256, (h, w)).astype(np.float32)
    d = ur.double_image(img8)
    assert np.array_equal(d[-1], d[-2]) and np.array_equal(d[:, -1], d[:, -2])
    d = ur.double_image(synth.texture(w + 16, h + 16, seed=3)[:h, :w])
    assert np.array_equal(d[-1, 0::2], d[-2, 0::2]) and np.array_equal(d[0::2, -1], d[0::2, -2])


@functools.lru_cache(maxsize=None)
def _image(w, h):
    img = synth.texture(w, h, seed=7)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("s0", [0.5, 0.4])
@pytest.mark.parametrize("w,h", [(203, 131), (160, 120)])
def test_composed_planes_are_the_oracles_pyramid_of_the_doubled_image(w, h, s0):
    """No initial blur on either side (the oracle skips it at initialSigma <= 0.5, the contract at <= 1.0): the composition from the
    oracle's primitives is the oracle's own pyramid of double_image(img), plane for plane."""
    p = orc.HessAffParams.default()
    p.initialSigma = s0
    dims, planes = ur.planes(_image(w, h), p)
    pyr = orc.Pyramid(ur.double_image(_image(w, h)), p)
    assert pyr.n_oct == len(dims) == {203: 5, 160: 5}[w]
    assert dims[0] == (2 * w, 2 * h)
    for o in range(pyr.n_oct):
        assert pyr.dims(o) == dims[o]
        for lv in range(p.numberOfScales + 2):
            for kind in (0, 1):
                assert np.array_equal(planes[(o, lv, kind)], pyr.plane(o, lv, kind)), (o, lv, kind)


def test_the_library_exports_the_switch(pkg):
    lib = pkg.lib()
    for name in ("mods_ctx_upscale_input", "mods_ctx_upscale_input_get", "mods_pipeline_upscale_input", "mods_upscale2x"):
        assert hasattr(lib, name), name
    for cls, name in ((pkg.Context, "upscale_input"), (pkg.Context, "upscale2x"), (pkg.Pipeline, "upscale_input")):
        assert callable(getattr(cls, name, None)), name
