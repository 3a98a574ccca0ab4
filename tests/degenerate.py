"""Degenerate detector inputs: images whose responses tie, repeat or are constant along an axis - the opposite of synth.texture,
on which no two responses are equal.  Pure numpy, float32, values 0 / amp.  Test infrastructure only.

What each one is for (tests/test_cpu_degenerate.py holds them to it):
  dots, tile_lattice  a lattice of period 3 makes almost every pixel an in-plane extremum: more than 768 per wave tile of
                      nms4_kernel, which is what makes that kernel empty its 1024-entry list in the middle of a level
  checker             thousands of keypoints whose |response| is shared bit for bit: every tie-break of the response order
  checker at 1e25     the Hessian response overflows: +inf next to +inf in the levels above and below, NaN where inf - inf - maxima
                      that tie ACROSS planes (only rejected by a neighbour strictly beyond them), NaN under the max / min forms
  stripes             constant along one axis: every pixel of a ridge is a 3x3x3 extremum (plateaux under the strict comparisons)
                      and every one of them is a singular system for the localisation
"""
import numpy as np

# nms4_kernel's wave geometry (csrc/detect.hip: NMS_ROWS, NMS4_COLS): a wave answers for 8 rows x 248 columns, the rows
# counted from the border, the columns from the plane's first
WAVE_ROWS, WAVE_COLS = 8, 248
# tile_lattice(.., 3, 255, LATTICE_SEED): 2208 candidates at 512x96 and, at 512x96 and 500x64, more than 100 octave-0 hits in wave tiles
# that hold more than 768 in-plane extrema
LATTICE_SEED = 3


def params(mod, det="hessian", mode=0, reg=-1, rel_th=-1.0, rel_n=-1.0):
    """the .ini parameters of a detector as `mod` (orc or the package) states them, with the key selection of `mode` when it is
    not the fixed threshold"""
    p = {"hessian": mod.HessAffParams.default, "dog": mod.HessAffParams.dog, "harris": mod.HessAffParams.harris}[det]()
    if mode:
        p.mode, p.regionsNumber, p.relativeThreshold, p.relativeRegionsNumber = mode, reg, rel_th, rel_n
    return p


def dots(w, h, P, amp):
    """single pixels of value amp every P pixels in both directions (the first at P // 2), on 0"""
    img = np.zeros((h, w), np.float32)
    img[P // 2::P, P // 2::P] = amp
    return img


def tile_lattice(w, h, P, amp, seed):
    """a random P x P tile of 0 / amp (neither all 0 nor all amp), repeated over the image"""
    rng = np.random.default_rng(seed)
    while True:
        tile = rng.integers(0, 2, (P, P))
        if 0 < tile.sum() < P * P:
            break
    reps = (-(-h // P), -(-w // P))
    return (np.tile(tile, reps)[:h, :w] * amp).astype(np.float32)


def checker(w, h, P, amp):
    """checkerboard of P x P squares, the square at the origin 0"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx // P) + (yy // P)) & 1) * amp).astype(np.float32)


def stripes(w, h, P, amp, vertical=True):
    """stripes of period P (P // 2 pixels of amp, the rest 0); vertical: constant along y"""
    n = w if vertical else h
    line = np.where(np.arange(n) % P < P // 2, amp, 0).astype(np.float32)
    return np.tile(line[None, :], (h, 1)) if vertical else np.tile(line[:, None], (1, w))


def inplane_extrema(plane, pos_th, neg_th, border):
    """The in-plane half of the 3x3x3 test as the detector states it: val > pos_th and no neighbour of the 3x3 block strictly
    larger, or else val < neg_th and none strictly smaller, for the pixels at least `border` from every edge."""
    p = np.asarray(plane, np.float32)
    h, w = p.shape
    q = np.pad(p, 1, mode="edge")          # the padded ring only reaches pixels that the border masks
    mx = np.full_like(p, -np.inf)
    mn = np.full_like(p, np.inf)
    for dr in range(3):
        for dc in range(3):
            s = q[dr:dr + h, dc:dc + w]
            mx = np.maximum(mx, s)
            mn = np.minimum(mn, s)
    cmax = (p > pos_th) & ~(mx > p)
    cmin = ~cmax & (p < neg_th) & ~(mn < p)
    hit = cmax | cmin
    inside = np.zeros_like(hit)
    inside[border:h - border, border:w - border] = True
    return hit & inside


def inplane_per_wave_tile(plane, pos_th, neg_th, border):
    """The largest number of in-plane extrema in one wave tile [border + 8k, +8) x [248j, 248j + 248) of the plane."""
    hit = inplane_extrema(plane, pos_th, neg_th, border)
    h, w = hit.shape
    best = 0
    for r in range(border, h - border, WAVE_ROWS):
        for c in range(0, w, WAVE_COLS):
            best = max(best, int(hit[r:min(r + WAVE_ROWS, h - border), c:c + WAVE_COLS].sum()))
    return best


def shared_response_fraction(keys):
    """fraction of the keys whose |response| equals another key's bit for bit"""
    if len(keys) == 0:
        return 0.0
    a = np.abs(np.asarray(keys["response"], np.float64))
    _, inv, cnt = np.unique(a, return_inverse=True, return_counts=True)
    return float((cnt[inv] > 1).mean())


def cross_plane_ties(pyr, raw):
    """(maxima, minima) among the raw hits `raw` of the oracle pyramid `pyr` whose response equals one of the 18 neighbours in the
    level below or above: hits that a non-strict comparison against the other planes would lose"""
    nmax = nmin = 0
    planes = {}
    for o, lv, r, c in np.asarray(raw).tolist():
        for q in (lv - 1, lv, lv + 1):
            if (o, q) not in planes:
                planes[(o, q)] = pyr.plane(o, q, 1)
        v = planes[(o, lv)][r, c]
        tie = any((planes[(o, q)][r - 1:r + 2, c - 1:c + 2] == v).any() for q in (lv - 1, lv + 1))
        nmax += int(tie and v > 0)
        nmin += int(tie and v < 0)
    return nmax, nmin
