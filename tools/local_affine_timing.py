#!/usr/bin/env python3
"""The local affine consistency filter (csrc/local_affine.hip) measured on the GPU; prints the text of
profiles/local_affine_timing.txt.  Stage times are the context's HIP-event stage timing ("local_affine": the fill, prep, both
sweeps, keep and the compaction), means over `reps` calls after one warm-up call per shape.
  - the standalone filter on synthetic planar scenes (tests/local_affine_ref.py: planar_scene) of 3 000, 20 000 and 150 000
    tentatives, in the generator's random list order and with the same list ordered by image-1 grid cells of side `radius` (what the
    sweep's tile skipping needs to take effect);
  - graf1 / graf6: tentatives, tentatives that follow the pair's homography, RANSAC samples - filter off and on at radius 60, 100, 160;
  - bench.py's harder_verification pair shape (40 % of image 2 follows the homography) through the pipeline, filter off and on.
python tools/local_affine_timing.py [reps]            the whole text
python tools/local_affine_timing.py --kernels N       only 20 filter calls on N tentatives (to be run under a kernel trace)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import local_affine_ref as lr  # noqa: E402
import synth  # noqa: E402

SHAPES = ((3000, 1920, 1080), (20000, 1920, 1080), (150000, 4096, 4096))


def scene(n, w, h, seed=1):
    return lr.planar_scene(n, 0.1, w, h, seed=seed, laf_noise=0.05, pos_noise=0.5)


def cell_order(laf, radius):
    cx = np.floor(laf[:, 0] / radius).astype(np.int64); cy = np.floor(laf[:, 1] / radius).astype(np.int64)
    return np.argsort(cy * (cx.max() + 1) + cx, kind="stable")


def timed_filter(pkg, ctx, tent, u6, laf, par, reps):
    out = ctx.filter_local_affine(tent, u6, laf, par)         # warm-up: the scratch grows here
    ctx.timing_enable(["local_affine"]); ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = ctx.filter_local_affine(tent, u6, laf, par)
    wall = (time.perf_counter() - t0) / reps * 1e3
    ms, n, _ = ctx.timing_read("local_affine")
    ctx.timing_enable([])
    return ms / reps, wall, out


def standalone(pkg, ctx, reps):
    par = pkg.LocalAffineParams.default(radius=100.0)
    print("standalone filter, radius 100 and the defaults otherwise, synthetic planar scenes with 10 % inliers; stage = HIP events around the filter's")
    print("launches, call = host clock around mods_filter_local_affine (pack, upload, launches, the wait, copy back)")
    for n, w, h in SHAPES:
        tent, u6, laf, is_true = scene(n, w, h)
        r = max(2, reps if n < 100000 else reps // 3)
        ms, wall, out = timed_filter(pkg, ctx, tent, u6, laf, par, r)
        kept = out[3]["keep"]
        o = cell_order(laf, par.radius)
        ms2, wall2, out2 = timed_filter(pkg, ctx, tent[o], u6[o], laf[o], par, r)
        assert np.array_equal(out2[3]["keep"], kept[o]), "the kept set depends on the list order"
        print("n = %6d in %d x %d: list order  stage %9.3f ms (%.3g pairs/s), call %9.3f ms; kept %d, true among them %d of %d"
              % (n, w, h, ms, n * n / (ms * 1e-3), wall, kept.sum(), (kept & is_true).sum(), is_true.sum()))
        print("             %s  cell order  stage %9.3f ms (%.3g pairs/s), call %9.3f ms; the same kept set"
              % (" " * len("%d x %d" % (w, h)), ms2, n * n / (ms2 * 1e-3), wall2))
    print()


def graf(pkg, reps):
    import torch
    from PIL import Image
    import orc
    g = [orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", n)).convert("RGB"))) for n in ("graf1.png", "graf6.png")]
    h, w = g[0].shape
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    img = torch.from_numpy(np.stack(g)).cuda()
    torch.cuda.synchronize()
    for name, steps in (("one view", [pkg.LadderStep.make((1,), 360.0)]), ("both HessianAffine steps of the MODS ladder", pkg.iters_mods_steps())):
        rows = []
        H = None
        for p in (None, dict(radius=60.0), dict(radius=100.0), dict(radius=160.0), dict(radius=160.0, minSupport=2, keepSparse=0)):
            ctx.set_local_affine(pkg.LocalAffineParams.default(**p) if p is not None else None)
            rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
            par = pkg.PairParams.default()
            pkg.ransac_pin_seed(4242)
            res, _ = pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, steps, rep1, rep2, par, min_matches=1 << 30)
            if H is None:
                H = list(res.H)          # the ground truth: the homography the unfiltered run verifies, as the ground-truth tests take it
            rep1.clear(); rep2.clear()
            par.ransac.groundTruth = 1
            for i, v in enumerate(H):
                par.ransac.gtH[i] = v
            pkg.ransac_pin_seed(4242)
            gt, _ = pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, steps, rep1, rep2, par, min_matches=1 << 30)
            rep1.close(); rep2.close()
            rows.append((p, res, gt))
        print("graf1 / graf6, %s (duplicates filtered first, 2 px, bestFGINN; true = within 4 px of the unfiltered run's H):" % name)
        for p, res, gt in rows:
            label = "filter off" if p is None else ", ".join("%s %g" % kv for kv in p.items())
            print("  %-42s tentatives %5d, to RANSAC %5d, true among them %5d, RANSAC samples %6d, inliers %4d"
                  % (label, res.n_tentatives, res.n_unique, gt.gt_true, res.ransac_samples, res.n_inliers))
    pkg.ransac_pin_seed(-1)
    ctx.set_local_affine(None)
    ctx.close()
    print()


def pipeline(pkg, n_pairs=256):
    import torch
    W, H = 1920, 1080
    hp = [synth.pair_partial(W, H, seed=2900 + i, frac=0.4) for i in range(3)]
    bufs = []
    for a_, b_, _ in hp:
        buf = pkg.PinnedBuffer((2, H, W), np.uint8)
        buf.array[...] = np.stack([a_, b_]).astype(np.uint8)
        bufs.append(buf)
    print("bench.py's harder_verification pairs (1920 x 1080, 40 % of image 2 follows the homography), 8-bit pinned host images, pipeline of")
    print("4 GPU workers x 16 pairs per batch + 8 verify workers, %d pairs after 64 of warm-up, alternating off / on / off / on:" % n_pairs)
    for rnd in range(2):
        for p in (None, pkg.LocalAffineParams.default()):
            pipe = pkg.Pipeline(0, W, H, pkg.PairParams.default(), 4, 8, 16, local_affine=p)

            def run(n):
                out, pending = [], 0
                for i in range(n):
                    if pending >= pipe.capacity - 1:
                        out.append(pipe.next()[0]); pending -= 1
                    pipe.submit_host(bufs[i % len(bufs)].ptr.value, i, u8=True); pending += 1
                while pending:
                    out.append(pipe.next()[0]); pending -= 1
                return out
            run(64)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = run(n_pairs)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            pipe.close()
            k = float(len(res))
            print("  filter %-3s %7.1f pairs/s; per pair: tentatives %6.1f, to RANSAC %6.1f, RANSAC samples %6.1f, inliers %6.1f, verification %.3f ms (RANSAC) + %.3f ms (duplicates)"
                  % ("on" if p is not None else "off", k / dt, sum(r.n_tentatives for r in res) / k, sum(r.n_unique for r in res) / k,
                     sum(r.ransac_samples for r in res) / k, sum(r.n_inliers for r in res) / k, sum(r.ms_ransac for r in res) / k,
                     sum(r.ms_duplicates for r in res) / k))
    for b in bufs:
        b.close()
    print()


def main():
    pkg = ge.load_package()
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        n = int(sys.argv[2])
        ctx = pkg.Context(0, 1920, 1080, 2)
        tent, u6, laf, _ = scene(n, 1920, 1080)
        par = pkg.LocalAffineParams.default(radius=100.0)
        for _ in range(20):
            ctx.filter_local_affine(tent, u6, laf, par)
        ctx.close()
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = pkg.Context(0, 1920, 1080, 2)
    standalone(pkg, ctx, reps)
    ctx.close()
    graf(pkg, reps)
    pipeline(pkg)


if __name__ == "__main__":
    main()
