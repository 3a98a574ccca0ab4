"""The degenerate images of tests/degenerate.py do what tests/test_gpu_detect_degenerate.py needs them for.  Oracle only: these are
conditions on the inputs, not on the code under test - a changed generator that no longer reaches nms4_kernel's mid-level flush, the
tie-breaks or the plateaux fails here, on the CPU, instead of quietly turning the GPU cases into easy ones."""
import numpy as np
import pytest

import degenerate as dg
import orc
from degenerate import LATTICE_SEED

def params(*a, **kw):
    return dg.params(orc, *a, **kw)


def _gates(p):
    th = 0.0 if p.mode else float(np.float32(0.8 * p.threshold))     # pyramid.h:46-59
    return th, -th


def _octave0_tiles(img, p):
    """per detection level of octave 0: (largest in-plane count of a wave tile, oracle hits that lie in tiles above 768)"""
    pyr = orc.Pyramid(img, p)
    _, raw = pyr.candidates()
    pos, neg = _gates(p)
    out = []
    for lv in range(1, p.numberOfScales + 1):
        ext = dg.inplane_extrema(pyr.plane(0, lv, 1), pos, neg, p.border)
        hits = raw[(raw[:, 0] == 0) & (raw[:, 1] == lv)]
        behind = 0
        for r, c in hits[:, 2:]:
            r0 = p.border + (r - p.border) // dg.WAVE_ROWS * dg.WAVE_ROWS
            c0 = c // dg.WAVE_COLS * dg.WAVE_COLS
            behind += int(ext[r0:min(r0 + dg.WAVE_ROWS, ext.shape[0] - p.border), c0:c0 + dg.WAVE_COLS].sum() > 768)
        out.append((dg.inplane_per_wave_tile(pyr.plane(0, lv, 1), pos, neg, p.border), behind))
    return out, pyr


def test_generators():
    d = dg.dots(10, 7, 3, 255)
    assert d.dtype == np.float32 and d.shape == (7, 10) and d.sum() == 255 * 6 and d[1, 1] == 255 and d[4, 7] == 255
    t = dg.tile_lattice(11, 8, 3, 255, LATTICE_SEED)
    assert t.dtype == np.float32 and np.array_equal(t[3:, 3:], t[:-3, :-3]) and set(np.unique(t)) == {0.0, 255.0}
    c = dg.checker(13, 12, 6, 1.0)
    assert c.dtype == np.float32 and c[0, 0] == 0 and c[0, 6] == 1 and c[6, 0] == 1 and c[6, 6] == 0 and c[5, 12] == 0
    v, hz = dg.stripes(24, 5, 12, 255, True), dg.stripes(5, 24, 12, 255, False)
    assert v.dtype == np.float32 and np.array_equal(v, hz.T) and np.array_equal(v[0], v[4])
    assert list(v[0, :13]) == [255] * 6 + [0] * 6 + [255]


def test_inplane_per_wave_tile_counts_by_hand():
    """a plane with known extrema: strict rejection only (plateaux count), maxima need > pos_th, minima < neg_th, the border masks,
    tiles are 8 rows from the border x 248 columns from column 0"""
    p = np.zeros((30, 600), np.float32)
    p[6, 10] = 5; p[6, 11] = 5               # a plateau of two maxima: both count (no neighbour strictly larger)
    p[7, 300] = -4                           # a minimum, in the second column tile
    p[13, 20] = 5                            # second row tile (rows 13 .. 20 with border 5)
    p[2, 50] = 9; p[20, 597] = 9             # inside the border: masked
    ext = dg.inplane_extrema(p, 1.0, -1.0, 5)
    assert int(ext.sum()) == 4 and ext[6, 10] and ext[6, 11] and ext[7, 300] and ext[13, 20]
    assert dg.inplane_per_wave_tile(p, 1.0, -1.0, 5) == 2
    assert dg.inplane_per_wave_tile(p, 6.0, -6.0, 5) == 0                 # the gates
    # gates of 0 (modes 1-4): the zero background is neither above 0 nor below 0, so it stays out
    assert dg.inplane_per_wave_tile(p, 0.0, 0.0, 5) == 2


@pytest.mark.parametrize("name", ["dots", "lattice"])
def test_lattices_reach_the_mid_level_flush(name):
    """more than 768 in-plane extrema in one wave tile of a detection level of octave 0 (nms4_kernel flushes its 1024-entry list
    when a row starts above 1024 - 4 * 64): at 512x96 and at 500x64; the lattice also gives >= 100 candidates, and true hits in the
    tiles that flush (a flush that lost entries would lose hits, not only rejected extrema)"""
    for w, h in ((512, 96), (500, 64)):
        img = dg.dots(w, h, 3, 255) if name == "dots" else dg.tile_lattice(w, h, 3, 255, LATTICE_SEED)
        p = params(mode=2, reg=100000)
        tiles, pyr = _octave0_tiles(img, p)
        assert max(t for t, _ in tiles) > 768, tiles
        if name == "lattice":
            cand, raw = pyr.candidates()
            assert len(cand) >= 100
            assert sum(b for _, b in tiles) >= 100, tiles


CHECKERS = [("p6_w500", 500, 6, 255.0, params()), ("p6_w501", 501, 6, 255.0, params()),
            ("p7_w500", 500, 7, 255.0, params()), ("p8_dog", 500, 8, 255.0, params("dog")),
            ("p6_unit_mode1", 500, 6, 1.0, params(mode=1, reg=5000, rel_th=0.5, rel_n=1.0))]


@pytest.mark.parametrize("case", CHECKERS, ids=[c[0] for c in CHECKERS])
def test_checkerboards_tie(case):
    _, w, P, amp, p = case
    keys = orc.detect_hessian_affine(dg.checker(w, 300, P, amp), p)
    assert len(keys) >= 1000
    assert dg.shared_response_fraction(keys) >= 0.9


def test_unit_checkerboard_has_cell_collisions():
    """0 / 1 checkerboard, mode 1: fewer candidates than raw hits - hits that localise to the same cell and lose it"""
    p = params(mode=1, reg=5000, rel_th=0.5, rel_n=1.0)
    cand, raw = orc.Pyramid(dg.checker(500, 300, 6, 1.0), p).candidates()
    assert len(cand) < len(raw)


@pytest.mark.parametrize("w", [252, 253])
def test_saturated_checkerboard_ties_across_levels(w):
    """checker at 1e25 under the Hessian: more than 1000 maxima and more than 1000 minima equal a neighbour in the level below or
    above (+-inf), the planes hold NaN, and no hit survives localisation (nothing with such values reaches the shape iteration)"""
    p = params()
    pyr = orc.Pyramid(dg.checker(w, 100, 6, 1e25), p)
    cand, raw = pyr.candidates()
    nmax, nmin = dg.cross_plane_ties(pyr, raw)
    assert nmax > 1000 and nmin > 1000 and len(cand) == 0
    assert np.isnan(pyr.plane(0, 1, 1)).any()
    assert any(np.isinf(pyr.plane(o, lv, 1)[r, c]) for o, lv, r, c in raw.tolist())


def test_stripes_are_all_plateau_and_all_rejected():
    p = params("dog")
    cand, raw = orc.Pyramid(dg.stripes(500, 300, 12, 255, True), p).candidates()
    assert len(raw) > 20000 and len(cand) == 0
    # the raw list is in processing order: octave, level, raster of (r0, c0) - what the GPU's lists are sorted into
    assert np.array_equal(np.lexsort((raw[:, 3], raw[:, 2], raw[:, 1], raw[:, 0])), np.arange(len(raw)))


def test_large_stripes_overflow_a_65536_entry_list():
    _, raw = orc.Pyramid(dg.stripes(640, 512, 12, 255, True), params("dog")).candidates()
    assert len(raw) > 65536
