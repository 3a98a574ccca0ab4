"""The spatial selection of a count-limited detector's regions (include/mods_hip.h: mods_ctx_spatial_selection) restated in numpy.
Nothing here knows how the GPU computes it: every operation is a numpy float32 operation, rounded on its own.  Below the contract:
the constructed key lists the CPU and the GPU tests share."""
import numpy as np


def keep_count(mode, n, regions_number=0, relative_regions_number=0.0):
    """the count the cut of a count mode keeps of n keys: mode 2 FixedRegNumber, 3 RelativeRegNumber"""
    if mode == 2:
        keep = min(n, int(regions_number))
    elif mode == 3:
        keep = int(np.floor(np.float64(np.float32(relative_regions_number)) * np.float64(n)))
    else:
        raise ValueError("the selection covers FixedRegNumber (2) and RelativeRegNumber (3)")
    return max(0, min(keep, n))


def radii(x, y, response, robustness):
    """r2[i] of the contract for a list in export order, float32; +inf where no key suppresses i"""
    xf = np.asarray(x).astype(np.float32)
    yf = np.asarray(y).astype(np.float32)
    a = np.abs(np.asarray(response).astype(np.float32))
    ca = np.float32(robustness) * a                       # float32 * float32 array: one rounding
    assert ca.dtype == np.float32
    n = len(a)
    r2 = np.full(n, np.inf, np.float32)
    for i0 in range(0, n, 256):                           # 256 rows of the all-pairs table at a time
        i1 = min(n, i0 + 256)
        sup = ca[None, :] > a[i0:i1, None]
        sup[np.arange(i1 - i0), np.arange(i0, i1)] = False
        cols = np.flatnonzero(sup.any(axis=0))            # (the columns that suppress none of these rows add nothing)
        if len(cols) == 0:
            continue
        dx = xf[i0:i1, None] - xf[None, cols]
        dy = yf[i0:i1, None] - yf[None, cols]
        d2 = dx * dx + dy * dy                            # float32 products, float32 sum
        assert d2.dtype == np.float32
        d2[~sup[:, cols]] = np.inf
        r2[i0:i1] = d2.min(axis=1)
    return r2


def pick(r2, keep):
    """the keep indices with the largest r2, ties to the smaller index, in increasing order"""
    n = len(r2)
    keep = max(0, min(int(keep), n))
    if keep <= 0 or keep >= n:
        return np.arange(keep, dtype=np.int64)
    key = ((~np.ascontiguousarray(r2, np.float32).view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return np.sort(np.argsort(key, kind="stable")[:keep]).astype(np.int64)


def select(x, y, response, keep, robustness):
    """the indices the selection keeps of the list, increasing; keep is clamped to [0, n]"""
    n = len(np.asarray(response))
    keep = max(0, min(int(keep), n))
    if keep <= 0 or keep >= n:
        return np.arange(keep, dtype=np.int64)
    return pick(radii(x, y, response, robustness), keep)


def select_keys(keys, keep, robustness):
    """select() on a structured key list (fields x, y, response); returns the kept keys"""
    return keys[select(keys["x"], keys["y"], keys["response"], keep, robustness)]


# ---- constructed lists: (x, y, response), |response| descending
def random_list(n, seed, w=640, h=480):
    """float positions in a w x h frame, distinct |responses| of mixed sign"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, w, n).astype(np.float32)
    y = rng.uniform(0, h, n).astype(np.float32)
    a = np.linspace(2000.0, 1.0, n).astype(np.float32) if n > 1 else np.array([2000.0], np.float32)
    assert len(np.unique(a)) == n
    return x, y, a * rng.choice(np.array([-1, 1], np.float32), n)


def lattice_list(seed=1):
    """every point of a 32 x 32 integer lattice once, in random order: many equal radii"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:32, 0:32]
    p = rng.permutation(1024)
    return xx.ravel()[p].astype(np.float32), yy.ravel()[p].astype(np.float32), np.linspace(500.0, 1.0, 1024).astype(np.float32)


def tied_response_list(n=500, block=10, seed=2):
    """blocks of `block` keys of one |response|, signs mixed"""
    x, y, _ = random_list(n, seed)
    rng = np.random.default_rng(seed + 1)
    a = (100.0 - (np.arange(n) // block)).astype(np.float32)
    return x, y, a * rng.choice(np.array([-1, 1], np.float32), n)


def duplicate_position_list(n=600, unique=200, seed=3):
    """every position `n / unique` times: radii of 0"""
    x, y, r = random_list(n, seed)
    rng = np.random.default_rng(seed + 1)
    src = rng.integers(0, unique, n)
    return x[src], y[src], r


def equal_radius_list(copies=5):
    """one strong key at (320, 240) and the 20 lattice points at distance 25 of it, each `copies` times, with responses so close that
    at robustness 0.9 only the strong key suppresses them: every radius but the first is 625"""
    pts = [(25, 0), (0, 25), (7, 24), (24, 7), (15, 20), (20, 15)]
    ring = sorted({(sx * px, sy * py) for px, py in pts for sx in (-1, 1) for sy in (-1, 1)})
    assert len(ring) == 20 and all(px * px + py * py == 625 for px, py in ring)
    ring = np.array(ring * copies, np.float32)
    n = len(ring)
    x = np.concatenate([[320.0], 320.0 + ring[:, 0]]).astype(np.float32)
    y = np.concatenate([[240.0], 240.0 + ring[:, 1]]).astype(np.float32)
    r = np.concatenate([[1000.0], np.linspace(10.5, 10.0, n)]).astype(np.float32)
    return x, y, r


def clustered_scene(seed=4):
    """300 strong keys inside the 10 x 10 px square at (100, 100), then 100 weaker ones on a 50 px lattice elsewhere"""
    rng = np.random.default_rng(seed)
    xs = rng.uniform(100, 110, 300).astype(np.float32)
    ys = rng.uniform(100, 110, 300).astype(np.float32)
    gy, gx = np.mgrid[0:10, 0:10]
    xw = (150 + 50 * gx.ravel()).astype(np.float32)
    yw = (20 + 50 * gy.ravel()).astype(np.float32)
    p = rng.permutation(100)
    r = np.concatenate([np.linspace(1000.0, 701.0, 300), np.linspace(100.0, 1.0, 100)]).astype(np.float32)
    return np.concatenate([xs, xw[p]]), np.concatenate([ys, yw[p]]), r
