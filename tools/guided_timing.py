#!/usr/bin/env python3
"""Guided matching (csrc/guided.hip) timed with the context's stage timing (HIP events around the whole search: pack, both gate
sweeps, accept, compaction, emit), the FGINN match stage at the same shape beside it as the yardstick, in one run:
  - synthetic lists of 60 156 x 47 177 regions in a 1920 x 1080 frame (the size of the matcher's roofline leg), H and F mode;
  - the banks the MODS ladder leaves for graf1 / graf6 (both HessianAffine steps run), H from the ladder, F from DEGENSAC on the
    guided matches.
Prints the profile text (profiles/guided_timing.txt).  python tools/guided_timing.py [reps]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import test_gpu_guided as tg  # noqa: E402  (the scene generators)


def timed(pkg, ctx, stage, fn, reps):
    fn()                                     # warm-up: buffers grow here
    ctx.timing_enable([stage]); ctx.timing_reset()
    for _ in range(reps):
        out = fn()
    ms, n, _ = ctx.timing_read(stage)
    ctx.timing_enable([])
    return ms / reps, out


def main():
    import torch
    from PIL import Image
    import orc
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    pkg = ge.load_package()
    d = pkg.view_ctx_dims(800, 640)
    ctx = pkg.Context(0, max(d[0], 1920), max(d[1], 1080), 2)
    print("guided matching, stage timing (HIP events, mean of %d calls after one warm-up); FGINN = the match stage of" % reps)
    print("mods_match_reps (ratio 0.8, nn 50) on the same banks in the same run")
    print()
    rng = np.random.default_rng(5)
    F, transfer = tg.fundamental(rng)
    for mode, model, tr, name in ((0, tg.H_PROJ.reshape(9), tg.H_PROJ, "H"), (1, F, transfer, "F")):
        q, t = tg.scene(rng, 60156, 47177, tr, w=1920.0, h=1080.0, noise=2.0)
        rq, rt = pkg.ImgRep(ctx, len(q)), pkg.ImgRep(ctx, len(t))
        rq.append_host(q); rt.append_host(t)
        for radius in (4.0, 16.0):
            p = pkg.GuidedParams.default(model, model_type=mode, radius=radius, ratio=0.9, contrad=10.0, one_to_one=1)
            ms, out = timed(pkg, ctx, "guided", lambda: pkg.match_guided_reps(ctx, rq, rt, p), reps)
            print("synthetic %d x %d, %s mode, radius %4.1f: guided %.3f ms, %d correspondences" % (len(q), len(t), name, radius, ms, len(out[0])))
        ms, out = timed(pkg, ctx, "match", lambda: pkg.match_reps(ctx, rq, rt), reps)
        print("synthetic %d x %d, FGINN yardstick:        match  %.3f ms, %d tentatives" % (len(q), len(t), ms, len(out[0])))
        rq.close(); rt.close()
    print()
    g = [orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", n)).convert("RGB"))) for n in ("graf1.png", "graf6.png")]
    h, w = g[0].shape
    img = torch.from_numpy(np.stack(g)).cuda()
    torch.cuda.synchronize()
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
    pkg.ransac_pin_seed(4242)
    res, _ = pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, pkg.iters_mods_steps(), rep1, rep2, pkg.PairParams.default(), min_matches=1 << 30)
    H = np.array(list(res.H))
    print("graf1 / graf6, MODS ladder (both HessianAffine steps): banks %d x %d, %d tentatives, %d unique, %d RANSAC inliers"
          % (len(rep1), len(rep2), res.n_tentatives, res.n_unique, res.n_inliers))
    p = pkg.GuidedParams.default(H, radius=4.0, ratio=0.9, contrad=10.0, one_to_one=1)
    ms, out = timed(pkg, ctx, "guided", lambda: pkg.match_guided_reps(ctx, rep1, rep2, p), reps)
    dd = pkg.duplicate_filter_gpu(ctx, out[0], out[1], out[2], 2.0, 1)
    print("  H mode, radius 4, ratio 0.9, one to one: guided %.3f ms, %d correspondences, %d after duplicate filtering (2 px, bestFGINN)"
          % (ms, len(out[0]), len(dd[0])))
    _, Fg, n_f, _ = pkg.loransac_f(dd[1], dd[2], seed_time=4242)
    p = pkg.GuidedParams.default(Fg, model_type=1, radius=4.0, ratio=0.9, contrad=10.0, one_to_one=1)
    ms, out = timed(pkg, ctx, "guided", lambda: pkg.match_guided_reps(ctx, rep1, rep2, p), reps)
    dd = pkg.duplicate_filter_gpu(ctx, out[0], out[1], out[2], 2.0, 1)
    print("  F mode (DEGENSAC on the guided set, %d inliers), radius 4: guided %.3f ms, %d correspondences, %d after duplicate filtering"
          % (n_f, ms, len(out[0]), len(dd[0])))
    ms, out = timed(pkg, ctx, "match", lambda: pkg.match_reps(ctx, rep1, rep2), reps)
    print("  FGINN yardstick: match %.3f ms, %d tentatives" % (ms, len(out[0])))
    pkg.ransac_pin_seed(-1)
    rep1.close(); rep2.close(); ctx.close()


if __name__ == "__main__":
    main()
