#!/usr/bin/env python3
"""Overlap matching (csrc/overlap.hip) timed with the context's stage timing (HIP events around the whole search: pack, the sweep,
accept, compaction, emit), oriented and unoriented, with the guided search in H mode (radius 4) on the same banks in the same
run as the yardstick:
  - synthetic lists of 60 156 x 47 177 regions in a 1920 x 1080 frame (the size of the matcher's roofline leg; the scene of
    tests/overlap_ref.py, random descriptors for the guided search);
  - the banks the MODS ladder leaves for graf1 / graf6 (both HessianAffine steps run), H from the ladder.
Prints the profile text (profiles/overlap_timing.txt).  python tools/overlap_timing.py [reps]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import overlap_ref as orf  # noqa: E402  (the scene generator)


def timed(ctx, stage, fn, reps):
    fn()                                     # warm-up: buffers grow here
    ctx.timing_enable([stage]); ctx.timing_reset()
    for _ in range(reps):
        out = fn()
    ms, n, _ = ctx.timing_read(stage)
    ctx.timing_enable([])
    return ms / reps, out


def report(pkg, ctx, rq, rt, H, w, h, reps, name):
    for oriented in (1, 0):
        for one in (1, 0):
            p = pkg.OverlapParams.default(H, max_error=0.09, oriented=oriented, one_to_one=one, w1=w, h1=h, w2=w, h2=h)
            ms, (m, c) = timed(ctx, "overlap", lambda: pkg.match_overlap_reps(ctx, rq, rt, p), reps)
            print("%s, oriented %d, one to one %d: overlap %.3f ms, %d matches, common area %d | %d, repeatability %.4f"
                  % (name, oriented, one, ms, c.n_matches, c.n_q_common, c.n_t_common, c.repeatability))
    g = pkg.GuidedParams.default(H, radius=4.0, ratio=0.9, contrad=10.0, one_to_one=1)
    ms, out = timed(ctx, "guided", lambda: pkg.match_guided_reps(ctx, rq, rt, g), reps)
    print("%s, guided yardstick (H mode, radius 4, two gate sweeps): guided %.3f ms, %d correspondences" % (name, ms, len(out[0])))


def main():
    import torch
    from PIL import Image
    import orc
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    pkg = ge.load_package()
    d = pkg.view_ctx_dims(800, 640)
    ctx = pkg.Context(0, max(d[0], 1920), max(d[1], 1080), 2)
    print("overlap matching, stage timing (HIP events, mean of %d calls after one warm-up); guided = the guided search of" % reps)
    print("mods_match_guided_reps on the same banks in the same run")
    print()
    rng = np.random.default_rng(5)
    q, t = orf.scene(rng, 60156, 47177, orf.H_PROJ, w=1920.0, h=1080.0)
    q["desc"] = rng.integers(0, 256, (len(q), 128), dtype=np.uint8); t["desc"] = rng.integers(0, 256, (len(t), 128), dtype=np.uint8)
    rq, rt = pkg.ImgRep(ctx, len(q)), pkg.ImgRep(ctx, len(t))
    rq.append_host(q); rt.append_host(t)
    report(pkg, ctx, rq, rt, orf.H_PROJ, 1920, 1080, reps, "synthetic %d x %d" % (len(q), len(t)))
    p = pkg.OverlapParams.default(orf.H_PROJ, max_error=0.09, w1=1920, h1=1080, w2=1920, h2=1080)
    try:
        for splits in (1, 4, 16, 64):
            ctx.overlap_splits(splits)
            ms, _ = timed(ctx, "overlap", lambda: pkg.match_overlap_reps(ctx, rq, rt, p), reps)
            print("  the same with %2d train split(s): overlap %.3f ms" % (splits, ms))
    finally:
        ctx.overlap_splits(0)
    rq.close(); rt.close()
    print()
    g = [orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", n)).convert("RGB"))) for n in ("graf1.png", "graf6.png")]
    h, w = g[0].shape
    img = torch.from_numpy(np.stack(g)).cuda()
    torch.cuda.synchronize()
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
    pkg.ransac_pin_seed(4242)
    res, _ = pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, pkg.iters_mods_steps(), rep1, rep2, pkg.PairParams.default(), min_matches=1 << 30)
    pkg.ransac_pin_seed(-1)
    print("graf1 / graf6, MODS ladder (both HessianAffine steps): banks %d x %d, %d RANSAC inliers, H from the ladder"
          % (len(rep1), len(rep2), res.n_inliers))
    report(pkg, ctx, rep1, rep2, np.array(list(res.H)), w, h, reps, "  graf banks")
    rep1.close(); rep2.close(); ctx.close()


if __name__ == "__main__":
    main()
