"""numpy restatement of CLAHE on 8-bit grey images: the CPU path of OpenCV 3.x / 4.x imgproc/src/clahe.cpp for CV_8UC1, which
the [Matching] doCLAHE branch of mods.cpp:133-189 calls (createCLAHE(), setClipLimit(4), 8 x 8 tiles).  OpenCV is not available
here, so this file and csrc/clahe.hip are two statements of the same specification (parity unpinned):

  - the LUTs come from the image, or - when w % tiles_x or h % tiles_y is nonzero - from the image padded at the right by
    tiles_x - w % tiles_x columns and at the bottom by tiles_y - h % tiles_y rows with BORDER_REFLECT_101 (both dimensions grow
    when either is indivisible)
  - per tile: 256-bin histogram; clip = max(int(clip_limit * total / 256), 1) when clip_limit > 0; clipped counts redistributed
    (clipped // 256 to every bin, the residual one by one to bins 0, step, 2 step, ... with step = max(256 // residual, 1));
    lut = saturate(rint(float32(cumsum) * float32(255 / total)))
  - per pixel of the w x h image: bilinear blend of the four neighbouring tiles' LUTs in float32, one rounding per operation

tiles = (tiles_x, tiles_y).  No device is needed."""
import numpy as np


def tile_size(w, h, tiles_x, tiles_y):
    """(tile_w, tile_h) of the (padded) LUT source"""
    if w % tiles_x or h % tiles_y:
        w, h = w + tiles_x - w % tiles_x, h + tiles_y - h % tiles_y
    return w // tiles_x, h // tiles_y


def clip_count(clip_limit, total):
    return max(int(clip_limit * total / 256), 1) if clip_limit > 0 else 0


def reflect101(idx, n):
    """cv::borderInterpolate(idx, n, BORDER_REFLECT_101), repeated for pads longer than the image"""
    idx = np.asarray(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    while True:
        out = (idx < 0) | (idx >= n)
        if not out.any():
            return idx
        idx = np.where(idx < 0, -idx, np.where(idx >= n, 2 * n - 2 - idx, idx))


def luts(img, clip_limit=4.0, tiles=(8, 8)):
    """uint8 [tiles_y * tiles_x, 256]: the LUT of every tile, row-major over the grid"""
    img = np.asarray(img, np.uint8)
    tx_n, ty_n = tiles
    h, w = img.shape
    tw, th = tile_size(w, h, tx_n, ty_n)
    src = img[np.ix_(reflect101(np.arange(th * ty_n), h), reflect101(np.arange(tw * tx_n), w))]
    total = tw * th
    n_tiles = tx_n * ty_n
    t = src.reshape(ty_n, th, tx_n, tw).transpose(0, 2, 1, 3).reshape(n_tiles, total).astype(np.int64)
    hist = np.bincount((t + 256 * np.arange(n_tiles)[:, None]).ravel(), minlength=256 * n_tiles).reshape(n_tiles, 256)
    clip = clip_count(clip_limit, total)
    if clip > 0:
        clipped = np.maximum(hist - clip, 0).sum(1)
        hist = np.minimum(hist, clip) + (clipped // 256)[:, None]
        residual = clipped % 256
        step = np.maximum(256 // np.maximum(residual, 1), 1)[:, None]
        i = np.arange(256)[None, :]
        hist = hist + ((residual[:, None] > 0) & (i % step == 0) & (i // step < residual[:, None]))
    scale = np.float32(255.0) / np.float32(total)
    cum = np.cumsum(hist, 1).astype(np.float32)
    return np.clip(np.rint(cum * scale), 0, 255).astype(np.uint8)


def _axis(n, size, tiles):
    inv = np.float32(1.0) / np.float32(size)
    f = np.arange(n).astype(np.float32) * inv - np.float32(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = f - t1.astype(np.float32)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, np.float32(1.0) - a


def clahe(img, clip_limit=4.0, tiles=(8, 8)):
    """the equalised uint8 image"""
    img = np.asarray(img, np.uint8)
    tx_n, ty_n = tiles
    h, w = img.shape
    tw, th = tile_size(w, h, tx_n, ty_n)
    L = luts(img, clip_limit, tiles).reshape(ty_n, tx_n, 256).astype(np.float32)
    tx1, tx2, xa, xa1 = _axis(w, tw, tx_n)
    ty1, ty2, ya, ya1 = _axis(h, th, ty_n)
    v = img.astype(np.int64)
    r1, r2 = ty1[:, None], ty2[:, None]
    res = (L[r1, tx1[None, :], v] * xa1 + L[r1, tx2[None, :], v] * xa) * ya1[:, None] + \
          (L[r2, tx1[None, :], v] * xa1 + L[r2, tx2[None, :], v] * xa) * ya[:, None]
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)
