#!/usr/bin/env python3
"""Homography views (csrc/view_h.hip) timed with the context's stage timing (HIP events around the launches), in one run:
  - warp_perspective_kernel on a 1920 x 1080 image (mods_synth_view_h_dev without the blur: that one launch), next to ONE launch
    of warp_affine_kernel at the same size (mods_synth_view_dev on a geometry whose second warp is empty) as the yardstick;
  - the post-pass (reproject_regions_h_kernel) on 10 000 regions, with and without a twin list;
  - the whole rematch on graf1 / graf6 behind the one-view ladder (host clock around the call, which ends synchronised), with the
    counts before and after, and the synthetic pair of tests/test_gpu_view_h.py with its corner errors.
Prints the profile text (profiles/view_h_timing.txt).  python tools/view_h_timing.py [reps]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import test_gpu_view_h as tv  # noqa: E402  (the region lists, the pairs)


def timed(ctx, stage, fn, reps):
    fn()                                     # warm-up
    ctx.timing_enable([stage]); ctx.timing_reset()
    for _ in range(reps):
        out = fn()
    ms, n, _ = ctx.timing_read(stage)
    ctx.timing_enable([])
    return ms / reps, n // reps, out


def main():
    import torch
    import synth
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    pkg = ge.load_package()
    W, H = 1920, 1080
    ctx = pkg.Context(0, W, H, 1)
    print("homography views, stage timing (HIP events, mean of %d calls after one warm-up)" % reps)
    print()
    img = torch.from_numpy(synth.texture(W, H, seed=11)).cuda()
    dst = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # the same affine map through both kernels, and a projective one through the new kernel
    A = [0.98, 0.17, -60.0, -0.17, 0.98, 140.0]
    ga = pkg.ViewGeom()
    ga.identity, ga.w_rot, ga.h_rot, ga.w_new, ga.h_new = 0, W, H, 0, 0       # no second warp
    for i, v in enumerate(A):
        ga.warpRot[i] = v
    ms_a, n_a, _ = timed(ctx, "synth", lambda: ctx.synth_view_dev(img.data_ptr(), W, H, ga, dst.data_ptr(), do_blur=0), reps)
    px = W * H
    print("warp_affine_kernel      1920 x 1080 -> 1920 x 1080, rotation 10 deg (yardstick): %.4f ms, %d launch, %.0f GB/s of 8 B/pixel"
          % (ms_a, n_a, 8.0 * px / ms_a / 1e6))
    for name, Hm in (("the same affine map", A + [0.0, 0.0, 1.0]), ("projective (2.5e-4, -1.5e-4)", A + [2.5e-4 / 4, -1.5e-4 / 4, 1.0])):
        g = pkg.view_geometry_h(W, H, Hm, W, H, 0.2)
        g.w_new, g.h_new = W, H
        ms_h, n_h, _ = timed(ctx, "synth", lambda: ctx.synth_view_h_dev(img.data_ptr(), W, H, g, dst.data_ptr(), do_blur=0), reps)
        print("warp_perspective_kernel 1920 x 1080 -> 1920 x 1080, %-28s: %.4f ms, %d launch, %.0f GB/s, %.2f x the yardstick"
              % (name, ms_h, n_h, 8.0 * px / ms_h / 1e6, ms_h / ms_a))
    print()
    r = tv._regions(pkg, 10000, seed=77, lo=-0.05, hi=1.05, s_max=3.0)
    half = r.copy()
    for twins in (None, half):
        ms_p, n_p, out = timed(ctx, "reproject_h", lambda: ctx.reproject_regions_h(r, tv.PROJ, tv.OW, tv.OH, half=twins), reps)
        kept = len(out[0]) if twins is not None else len(out)
        print("reproject_regions_h_kernel, 10 000 regions%s: %.4f ms, %d launch, %d kept (one workgroup of 256, 40 chunks)"
              % (" + twin list" if twins is not None else "            ", ms_p, n_p, kept))
    ctx.close()
    print()

    def rematch(a, b, both, label, H_true=None):
        h, w = a.shape
        d = pkg.view_ctx_dims(w, h)
        c = pkg.Context(0, d[0], d[1], 1)
        rep1, rep2 = pkg.ImgRep(c), pkg.ImgRep(c)
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        step = [pkg.LadderStep.make((1,), 360.0, init_sigma=0.2)]
        ms = []
        for it in range(4):                       # the first round warms the buffers up
            rep1.clear(); rep2.clear()
            pkg.ransac_pin_seed(4242)
            t0 = time.perf_counter()
            first, _ = pkg.match_ladder_dev(c, t.data_ptr(), w, h, step, rep1, rep2, min_matches=15, max_matches=100000)
            t1 = time.perf_counter()
            n1, n2 = len(rep1), len(rep2)
            pkg.ransac_pin_seed(4242)
            again, m = pkg.rematch_under_h_dev(c, t.data_ptr(), w, h, t.data_ptr() + 4 * w * h, w, h, list(first.H), rep1, rep2, both=both,
                                               init_sigma=0.2, max_matches=100000)
            t2 = time.perf_counter()
            ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        pkg.ransac_pin_seed(-1)
        print("%s, both = %d: first pass %d | %d regions, %d tentatives, %d unique, %d verified; rematch +%d | +%d regions, %d tentatives, %d unique, "
              "%d verified" % (label, both, n1, n2, first.n_tentatives, first.n_unique, first.n_inliers, len(rep1) - n1, len(rep2) - n2,
                               again.n_tentatives, again.n_unique, again.n_inliers))
        print("    host clock, 3 rounds after a warm-up: first pass %s ms, rematch %s ms (of the last: match %.2f, duplicates %.2f, verification %.2f)"
              % (" ".join("%.2f" % x[0] for x in ms[1:]), " ".join("%.2f" % x[1] for x in ms[1:]), again.ms_match, again.ms_duplicates, again.ms_ransac))
        if H_true is not None:
            print("    largest corner transfer error against H_true: first pass %.4f px, rematch %.4f px"
                  % (tv._corner_error(list(first.H), H_true, w, h), tv._corner_error(list(again.H), H_true, w, h)))
        rep1.close(); rep2.close(); c.close()

    a, b = tv._grey(tv.G1), tv._grey(tv.G6)
    rematch(a, b, 0, "graf1 / graf6 (800 x 640), one view, seed 4242")
    rematch(a, b, 1, "graf1 / graf6 (800 x 640), one view, seed 4242")
    a, b, H_true = tv.synthetic_pair()
    rematch(a, b, 0, "synthetic pair (400 x 300 crop of graf1 and its restated warp)", H_true)


if __name__ == "__main__":
    main()
