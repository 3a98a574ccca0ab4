"""Reference for orientation + description at ARBITRARY mods_describe_params, composed of the oracle's single-step entry points
(orc.describe_rootsift and orc.detect_describe hard-code RootSIFT and maxBinValue = 0.2, oracle/describe.cpp:448):

    orc.detect_orientation(img, regs, ori_mrSize, ori_patchSize, ori_maxAngles, ori_threshold, half) -> orc.filter_touch_boundary
    -> per region orc.extract_desc_patch(img, r, desc_mrSize, desc_patchSize, photoNorm, fast) -> orc.sift_desc(patch, rootSift,
    maxBinValue) [+ orc.half_rootsift_patch(patch, maxBinValue)]

and the branch census of the GPU cases: which kernel form and which extraction branch every described region of a case takes,
from Python restatements of region_geom, the tap count, sift_col_span and ori_key_bytes with the limits read out of the sources
(test_gpu_describe_u8_keys._sift_constants), on the oracle's region list alone.

The oracle had run at one parameter set only.  Places where a parameter enters the reference, compared with oracle/describe.cpp
line by line before this module relied on it (no difference found):
  patchSize / mrSize of DetectOrientation      synth-detection.cpp:1054-1059 (patchImageSize = 2 * int(mrSize) + 1, imageToPatchScale
                                               in double), :1074 (float curr_sc = imageToPatchScale * s), :1076-1084 (border box
                                               k_sigma * s whatever mrSize is; int parameters, helpers.cpp:524-549)
                                               -> describe.cpp:235-251
  patchSize of EstimateDominantAnglesFunctor   synth-detection.cpp:846-852 (mask sigma pS / 3.0f), :867-869 (rows 1 .. pS - 2, all
                                               columns), helpers.cpp:442-461 (sigma2 = 2 sigma^2, r2 = (pS >> 1)^2)
                                               -> describe.cpp:181-202
  threshold                                    io_mods.cpp:737 (a float member), synth-detection.cpp:886-889 (float thresh *= double
                                               max_th), :828 (hist[b] >= threshold), :891-898 (half mode folds AFTER the threshold)
                                               -> describe.cpp:204-211, 215
  maxAngles                                    synth-detection.cpp:856-859, 907-926 (the first maxAngles peaks in bin order; the sorted
                                               copy is unused) -> describe.cpp:176, 212-219
  patchSize / mrSize of DescribeRegions        synth-detection.hpp:187-192 (float mrScale = ceil(s * mrSize), 2 * int(mrScale) + 1,
                                               float imageToPatchScale, > 0.4 compared in double), :195-214 (window + 2, sigma
                                               1.5f * scale, centre patchImageSize >> 1), :183 (mask sigma 0 -> 0.9 r2)
                                               -> describe.cpp:421-434, 406
  fast extraction                              synth-detection.hpp:242-245 (double mrScale = mrSize * s, 2 * int(mrScale) + 1, scale in
                                               double, then float) -> describe.cpp:409-414
  photoNorm                                    synth-detection.hpp:228-231, helpers.cpp:666-715 -> describe.cpp:435-438
  patchSize of the SIFT tables                 siftdesc.cpp:24-25 (halfSize = patchSize >> 1, step = 5 / (2 * halfSize) in float),
                                               :36-69 -> describe.cpp:289-304
  maxBinValue, useRootSIFT                     siftdesc.h:36 (double), io_mods.cpp:427, siftdesc.cpp:199-222 (RootSIFTnorm(double)),
                                               :247-262 (SIFTnorm(double): 512.0f * v + 0.5 in double) -> describe.cpp:381-399
  HalfSIFT                                     siftdesc.cpp:401-436 -> describe.cpp:373-380.  SIFTnorm(double) loops over the 128 entries
                                               of `vec` while the half vector holds 64 (siftdesc.cpp:251): HalfSIFT without RootSIFT
                                               reads past the vector in the reference, so only HalfRootSIFT has a reference.
"""
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import orc
import synth
from test_gpu_describe_u8 import _p2, _window_touches
from test_gpu_describe_u8_keys import (ROOT, _boundaries, _boundary_keys, _border_key, _fits, _fuse_rows, _iso_key, _n_tap, _s_of,
                                       _sift_constants, _sizes_at, _tap_boundaries)

DEFAULTS = dict(ori_mrSize=orc.ORI_MRSIZE, ori_patchSize=orc.ORI_PATCH, ori_maxAngles=orc.ORI_MAXANG, ori_threshold=orc.ORI_TH,
                desc_mrSize=orc.DESC_MRSIZE, desc_patchSize=orc.DESC_PATCH, photoNorm=1, rootSift=1, maxBinValue=0.2, ori_halfMode=0,
                halfDesc=0, fastExtraction=0)


def params(**kw):
    """a full parameter set: the defaults of config_affori_classic.ini with the given ones replaced"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def to_struct(pkg, par):
    p = pkg.DescribeParams.default()
    for name, v in par.items():
        setattr(p, name, v)
    return p


def oriented(img, keys, par):
    """the regions the description sees: DetectOrientation and the border filter (no descriptors; no function of the desc_ ones)"""
    h, w = img.shape
    regs = orc.regions_from_keys(keys)
    assert len(orc.filter_centres_inside(regs, w, h)) == len(regs)       # (the oracle's `parent` counts the centres inside)
    o = orc.detect_orientation(img, regs, par["ori_mrSize"], par["ori_patchSize"], par["ori_maxAngles"], par["ori_threshold"],
                               half=bool(par["ori_halfMode"]))
    return orc.filter_touch_boundary(o, w, h)


def patches_of(img, regs, par):
    """the patch of every region as DescribeRegions hands it to the descriptor, fp32 [n][ps][ps]"""
    ps = par["desc_patchSize"]
    with ThreadPoolExecutor(8) as pool:      # (the oracle's calls release the interpreter lock)
        out = list(pool.map(lambda i: orc.extract_desc_patch(img, regs[i:i + 1], par["desc_mrSize"], ps, bool(par["photoNorm"]),
                                                             fast=bool(par["fastExtraction"])), range(len(regs))))
    return np.stack(out) if out else np.zeros((0, ps, ps), np.float32)


def describe_patches(regs, patches, par):
    """-> regions with descriptors (and their HalfRootSIFT twins with halfDesc)"""
    full, half = regs.copy(), regs.copy()
    assert par["rootSift"] or not par["halfDesc"]     # (HalfSIFT without RootSIFT has no reference: module docstring)
    for i in range(len(regs)):
        full["desc"][i] = orc.sift_desc(patches[i], bool(par["rootSift"]), par["maxBinValue"])
        if par["halfDesc"]:
            half["desc"][i] = orc.half_rootsift_patch(patches[i], par["maxBinValue"])
    return (full, half) if par["halfDesc"] else full


def describe(img, keys, par):
    regs = oriented(img, keys, par)
    return describe_patches(regs, patches_of(img, regs, par), par)


# ---- restatements of the launch decisions ----------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(ROOT, "mods-light-zmq_amd", "csrc", name)).read()


def sift_col_span(ps):
    """sift_col_span (csrc/sift.hip): the widest span of positive column weights of a spatial bin, in float32 as there"""
    f32 = np.float32
    step = f32(5.0) / f32(2 * (ps >> 1))
    span = 0
    for bc in range(4):
        on = []
        for i in range(ps):
            x = f32(step * f32(i)); xi = int(x); w1 = f32(x - f32(xi)); w0 = f32(f32(1.0) - w1)
            if (xi - 1 == bc and w0 > 0) or (xi == bc and w1 > 0):
                on.append(i)
        if on:
            span = max(span, on[-1] - on[0] + 1)
    return span


def sift_form(ps):
    """which SIFT kernel launch_extract_and_sift starts for the full descriptor: 'wave16', 'wave18' or 'block'"""
    src = _src("sift.hip")
    assert len(re.findall(r"if \(span <= 16\)", src)) == 2 and re.search(r"constexpr int SW_CW = 18;", src)
    if ps > _sift_constants()["sift_block_ps"]:
        return "block"
    span = sift_col_span(ps)
    assert span <= 18, (ps, span)      # wider than the 18 columns the wave form holds: nothing would take such a patch size
    return "wave16" if span <= 16 else "wave18"


def wave_chunk_limit():
    """the largest patch size at which the photometric chunk [SW_R][SW_G] floats of sift_wave2_kernel is larger than the wave's pixel
    row of SW_R * ps + SW_CW + 2 float2 it aliases (s2_row_slots, csrc/sift.hip): up to there the row area is sized by the chunk"""
    src = _src("sift.hip")
    r, g, cw = (int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("SW_R", "SW_G", "SW_CW"))
    assert re.search(r"s2_row_slots\(int ps\) \{ return SW_R \* ps \+ SW_CW \+ 2 > SW_R \* SW_G / 2 \?", src)
    return max(ps for ps in range(9, 64, 2) if 2 * (r * ps + cw + 2) < r * g)


def ori_key_bytes(ps):
    """ori_key_bytes (csrc/describe.hip): bytes of a vote's (bin, place) word"""
    m = re.findall(r"int ori_key_bytes\(int ps\) \{ return ps \* \(ps - 2\) > (\d+) \? 4 : 2; \}", _src("describe.hip"))
    assert len(m) == 1
    return 4 if ps * (ps - 2) > int(m[0]) else 2


def ori_window_sides(keys, w, h, par):
    """bool [n][4]: which borders (0 left, 1 top, 2 right, 3 bottom) the orientation window of every key reaches - the corners of
    interpolateCheckBorders (helpers.cpp:524-549) for the patch DetectOrientation samples (synth-detection.cpp:1059, 1074, 1091-1097)"""
    f32 = np.float32
    ps = par["ori_patchSize"]
    i2p = float(2 * int(par["ori_mrSize"]) + 1) / float(ps)
    sc = (i2p * keys["s"]).astype(f32)
    half = f32(np.ceil(float(f32(ps)) / 2.0))
    fx, fy = keys["x"].astype(f32), keys["y"].astype(f32)
    a11, a12, a21, a22 = (keys[f].astype(f32) * sc for f in ("a11", "a12", "a21", "a22"))
    sides = np.zeros((len(keys), 4), bool)
    for sx, sy in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        imx = fx + (f32(sx) * half) * a11 + (f32(sy) * half) * a12
        imy = fy + (f32(sx) * half) * a21 + (f32(sy) * half) * a22
        sides |= np.stack([np.floor(imx) <= 0, np.floor(imy) <= 0, np.ceil(imx) >= w - 2, np.ceil(imy) >= h - 2], axis=1)
    return sides


BRANCHES = ("direct", "lds", "lds_sent_to_hbm", "fused", "phase_by_taps", "phase_by_size", "taps_from_slab")


def census(regs, w, h, par):
    """{branch: (regions whose window touches the border, regions whose window does not)} of the extraction for described regions:
      direct           scale <= 0.4: the patch is sampled from the image (extract_small_kernel's other branch)
      lds              extract_small_kernel with the blur (P2 <= SMALL_CAP and the taps fit)
      lds_sent_to_hbm  P2 <= SMALL_CAP but more taps than the LDS tier stages: classified into the HBM tier
      fused            big_fused_kernel
      phase_by_taps    P2 <= BIG_FUSE_P2 but more taps than BIG_FUSE_TAPS: sample / row-pass / col-res kernels
      phase_by_size    P2 > BIG_FUSE_P2: the same kernels
      taps_from_slab   of the two phase classes: more taps than TAPS_LDS, the row pass reads them from the slab
    plus 'lds<t>' per launch of the LDS tier and 'fused<r>' per row count of the fused kernel."""
    k = _sift_constants()
    ps, mr = par["desc_patchSize"], par["desc_mrSize"]
    assert not par["fastExtraction"]
    P2 = _p2(regs, ps, mr)
    touch, direct = _window_touches(regs, w, h, ps, mr)
    ntap = np.array([_n_tap(int(p), ps) for p in P2], np.int64)
    small = ~direct & (P2 <= k["small_cap"])
    lds = small & (ntap <= k["lds_taps"])
    hbm = ~direct & ~lds
    fused = hbm & (P2 <= k["fuse_p2"]) & (ntap <= k["fuse_taps"])
    phase = hbm & ~fused
    m = dict(direct=direct, lds=lds, lds_sent_to_hbm=small & ~lds, fused=fused, phase_by_taps=phase & (P2 <= k["fuse_p2"]),
             phase_by_size=phase & (P2 > k["fuse_p2"]), taps_from_slab=phase & (ntap > k["taps_lds"]))
    for t, (lo, hi) in enumerate(zip((0, k["t_lo"], k["t_mid"]), (k["t_lo"], k["t_mid"], k["small_cap"]))):
        m["lds%d" % t] = lds & (P2 > lo) & (P2 <= hi)
    rows = np.array([_fuse_rows(int(p), k["fuse_kb"]) for p in P2], np.int64)
    for r in sorted(set(rows[fused].tolist())):
        m["fused%d" % r] = fused & (rows == r)
    return {name: (int(np.count_nonzero(v & touch)), int(np.count_nonzero(v & ~touch))) for name, v in m.items()}


def assert_census(cen, named, each=4):
    """every branch a case is named for holds at least `each` described regions"""
    for name in named:
        assert sum(cen.get(name, (0, 0))) >= each, "branch %s: %s regions, census %s" % (name, cen.get(name), cen)


# ---- the inputs of the GPU cases (tests/test_gpu_describe_params.py), shared with the census test on the CPU ----------------------
@functools.lru_cache(None)
def texture(w, h, seed):
    img = synth.texture(w, h, seed=seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(None)
def detected(w, h, seed, every):
    """every n-th keypoint the detector finds on the texture"""
    return orc.detect_hessian_affine(texture(w, h, seed))[::every].copy()


FLAT_HALF, FLAT_S = 63, 8.0      # half side of the constant squares and the scale of the keys at their centres
FLAT_ORI_MRSIZE = 8.0


@functools.lru_cache(None)
def forms_image():
    """640 x 480 texture with two constant squares, all 0 and all 255.  A key of scale FLAT_S at the centre of a square has a
    description window (half side ceil(5.1962 * 8) + 1.5 = 43.5, at any rotation within 61.6 px of the centre) that is constant,
    while an orientation window of mrSize 8 (8.5 * 8 = 68 px) reaches the texture around the square: the orientation is found, the
    patch is flat."""
    img = synth.texture(640, 480, seed=51).copy()
    for cx, v in ((160, 0.0), (480, 255.0)):
        img[240 - FLAT_HALF:240 + FLAT_HALF + 1, cx - FLAT_HALF:cx + FLAT_HALF + 1] = v
    img.setflags(write=False)
    return img


@functools.lru_cache(None)
def forms_keys():
    """(detector output on forms_image, every 8th; the two keys of the constant squares)"""
    img = forms_image()
    det = orc.detect_hessian_affine(img)
    flat = np.concatenate([_iso_key(det[:1], cx, 240.0, FLAT_S) for cx in (160.0, 480.0)])
    return det[::8].copy(), flat


SIFT_FORMS = {9: "wave16", 39: "wave16", 41: "wave16", 43: "wave18", 45: "wave18", 47: "block", 63: "block"}


def limits_case(ps):
    """B: (img, keys, par, limits, sizes): both window sizes at every limit of _boundaries(ps) a 640 x 480 image has room for, each at
    the centre and next to a border"""
    img = texture(640, 480, 41)
    base = detected(640, 480, 41, 1)[:1].copy()
    limits = [b for b in _boundaries(ps)[:-1] if _fits(b, 640, 480)]
    # At ps = 9 the only window the direct branch takes has ceil(s * mrSize) = 1, a region of less than a fifth of a pixel, over
    # which the default orientation patch (32 samples across 11 * s) has no gradient above 1 and finds no angle: s is taken from the
    # upper end of its interval and the orientation (at every ps: the cases are built alike) samples 8 x 8 across 17 * s.
    ori = dict(mrsize=8.0, ps=8)
    keys, sizes = _boundary_keys(img, base, limits, ps, orc.DESC_MRSIZE, s_shift=0.45, ori=ori)
    # the first limit has the direct branch below it, which its last size alone would give two regions: two more of the same window
    # size at another scale (ceil(s * mrSize) is the same), at another place and beside another border
    s = _s_of(_sizes_at(limits[0])[0]) + 0.3 / orc.DESC_MRSIZE
    more = [_iso_key(base, 320.0 + 7.3, 240.0 - 5.6, s), _border_key(img, base, s, 2, ps, orc.DESC_MRSIZE, ori)]
    return img, np.concatenate([keys] + more), params(desc_patchSize=ps, ori_mrSize=8.0, ori_patchSize=8), limits, sizes


TAPS_MRSIZE = 12.0


def tap_limits_case():
    """B, ps = 9 at desc_mrSize = 12 on 1200 x 1200: the two tap limits a 640 x 480 image has no room for (n_tap 319|321 at
    P2 = 321|323, 1023|1025 at P2 = 1023|1025).  With mrSize 12 the border filter's box (5.1962 * s) is 0.43 of the window, so
    s ~ 42.6 passes it; such a window covers most of the image and reaches over its border wherever it lies."""
    img = texture(1200, 1200, 43)
    base = detected(640, 480, 41, 1)[:1].copy()
    limits = _tap_boundaries(9)[1:]
    keys, sizes = [], []
    # (and the size after the last one: four regions whose taps the row pass reads from the slab, not two)
    for b in limits + [limits[-1] + 4]:
        for P2 in (_sizes_at(b) if b in limits else (b,)):
            s = _s_of(P2, TAPS_MRSIZE)
            keys.append(_iso_key(base, 600.0, 600.0, s))
            keys.append(_border_key(img, base, s, len(sizes) % 4, 9, TAPS_MRSIZE))
            sizes.append(P2)
    return img, np.concatenate(keys), params(desc_patchSize=9, desc_mrSize=TAPS_MRSIZE), limits, sizes


def mrsize_case(mr):
    """C: ps = 41 at desc_mrSize mr.  12.0: a 720 x 720 image with keys beside all four borders in three sizes, whose windows - wider
    than the box the border filter tested - read outside the image in the LDS tier (P2 = 51), the fused tier (243) and the sample
    tier (1027)."""
    if mr != 12.0:
        return texture(640, 480, 45), detected(640, 480, 45, 8), params(desc_mrSize=mr)
    img = texture(720, 720, 47)
    base = detected(640, 480, 45, 1)[:1].copy()
    keys = [detected(640, 480, 45, 16)]
    for P2 in (51, 243, 1027):
        keys += [_border_key(img, base, _s_of(P2, mr), side, 41, mr) for side in range(4)]
    return img, np.concatenate(keys), params(desc_mrSize=mr)


ORI_BORDER_S = 4.0


def orientation_keys():
    """D: detector output (every 8th) and isotropic keys of scale 4, three beside each border, 7.9 * s from it: inside the border
    filter's box at any rotation (5.1962 * s * sqrt(2) = 7.35 * s), inside an orientation window of mrSize 8 (8.5 * s)"""
    det = detected(640, 480, 49, 8)
    d = 7.9 * ORI_BORDER_S
    at = [(d, y) for y in (120.5, 240.25, 360.0)] + [(x, d) for x in (160.5, 320.25, 480.0)]
    at += [(639 - d, y) for y in (120.5, 240.25, 360.0)] + [(x, 479 - d) for x in (160.5, 320.25, 480.0)]
    return np.concatenate([det] + [_iso_key(det[:1], x, y, ORI_BORDER_S) for x, y in at])
