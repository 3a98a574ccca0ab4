#!/usr/bin/env python3
"""The tile rasteriser (csrc/draw.hip) timed with device events on the context's stream, after a warm-up call per shape:
  - the region image of a full bank: the contours of N regions (21 segments each) on a 1920 x 1080 canvas, built on the device
    (mods_canvas_draw_regions: the contour kernel, the tile kernel and the read of the drop count);
  - the match images of M correspondences on a 1920 x 1080 pair (mods_draw_matches: both composed canvases, ellipses and centres;
    the host composes and stages the lists inside the timed window);
  - the same lists through mods_canvas_draw alone (staging copy + tile kernel).
Each row: the median and the minimum over the repetitions in ms, and elements x tiles per second at the median (a workgroup per
16 x 16 tile walks the whole list: elements x tiles is the work of the bounding-box tests).  There is one level of tiles; a coarse
level was not built.  Writes profiles/draw_timing.txt.  python tools/draw_timing.py [reps] [out]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402


def bank(pkg, n, w, h, seed):
    """n regions anywhere in the frame, s from 1.5 to 12 (3 s: 4.5 .. 36 px), anisotropy up to 3"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, pkg.REGION_DTYPE)
    r["x"], r["y"] = rng.uniform(0, w, n), rng.uniform(0, h, n)
    r["s"] = rng.uniform(1.5, 12.0, n)
    ang, st = rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 1.7, n)
    r["a11"], r["a12"], r["a21"], r["a22"] = np.cos(ang) * st, -np.sin(ang) / st, np.sin(ang) * st, np.cos(ang) / st
    r["id"] = np.arange(n)
    return r


def timed(torch, stream, fn, reps):
    fn()                                              # warm-up: code objects, buffer growth
    stream.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "draw_timing.txt")
    pkg = ge.load_package()
    if pkg.lib().mods_device_count() <= 0:
        raise SystemExit("draw_timing: no HIP device; nothing is measured without one")
    torch.cuda.init()
    w, h = 1920, 1080
    ctx = pkg.Context(0, w, h, 1)
    stream = torch.cuda.ExternalStream(ctx.stream)
    lines = ["# tools/draw_timing.py on %s: device events on the context's stream, 1 warm-up + %d timed calls per row"
             % (torch.cuda.get_device_name(0), reps),
             "call | shape | elements | tiles | median ms | min ms | elements x tiles / s at the median"]

    def say(call, shape, n_el, tiles, med, mn):
        lines.append("%s | %s | %d | %d | %.3f | %.3f | %.3e" % (call, shape, n_el, tiles, med, mn, n_el * tiles / (med * 1e-3)))
        print(lines[-1], flush=True)

    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    base = np.random.default_rng(0).integers(0, 256, (h, w), dtype=np.uint8)
    cv = pkg.Canvas(ctx, w, h).blit(base)
    for n in (10000, 50000):
        rep = pkg.ImgRep(ctx, n)
        rep.append_host(bank(pkg, n, w, h, seed=n))
        med, mn = timed(torch, stream, lambda: cv.draw_regions(rep, thickness=2), reps)
        say("mods_canvas_draw_regions", "%d regions, 1920 x 1080, thickness 2" % n, 21 * n, tiles, med, mn)
        rep.close()
    n_m = 3000
    b1, b2 = bank(pkg, n_m, w, h, seed=1), bank(pkg, n_m, w, h, seed=2)
    laf = np.zeros((n_m, 14))
    for o, b in ((0, b1), (7, b2)):
        for k, f in enumerate(("x", "y", "a11", "a12", "a21", "a22", "s")):
            laf[:, o + k] = b[f]
    s1, s2 = pkg.Canvas(ctx, w, h).blit(base), pkg.Canvas(ctx, w, h).blit(base[::-1].copy())
    par = pkg.DrawMatchesParams.default(np.eye(3), centers_only=0, reproject=0)
    el = [pkg.draw_matches_elems(i, w, h, w, h, laf, par) for i in (0, 1)]

    def both():
        o1, o2, _ = pkg.draw_matches(ctx, s1, s2, laf, par)
        o1.close(); o2.close()

    med, mn = timed(torch, stream, both, reps)
    t1 = ((2 * w + 20 + 15) // 16) * ((h + 15) // 16)
    t2 = ((w + 15) // 16) * ((2 * h + 20 + 15) // 16)
    lines.append("mods_draw_matches | %d correspondences, two 1920 x 1080 images, ellipses + centres, both canvases | %d + %d | %d + %d | %.3f | %.3f | %.3e"
                 % (n_m, len(el[0]), len(el[1]), t1, t2, med, mn, (len(el[0]) * t1 + len(el[1]) * t2) / (med * 1e-3)))
    print(lines[-1], flush=True)
    wide = pkg.Canvas(ctx, 2 * w + 20, h).fill(0xFFFFFF)
    med, mn = timed(torch, stream, lambda: wide.draw(el[0]), reps)
    say("mods_canvas_draw", "the side-by-side list of %d correspondences, %d x %d" % (n_m, 2 * w + 20, h), len(el[0]), t1, med, mn)
    for c in (cv, s1, s2, wide):
        c.close()
    ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
