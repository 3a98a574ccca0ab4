#!/usr/bin/env python3
"""The mutual check of the FGINN matcher (csrc/mutual.hip; mods_ctx_match_mutual) timed with the context's stage timing - HIP events
around the match stage, and around the check's own launches (counter reset, list, sweep) inside it - mean of `reps` calls after one
warm-up, modes 0 / 1 / 2 in one run on
  - synthetic lists of 60 156 x 47 177 regions in a 1920 x 1080 frame (the size of the matcher's roofline leg),
  - the banks the MODS ladder leaves for graf1 / graf6 (both HessianAffine steps run),
  - the two region lists of a 1080p pair (synth.pair),
and what the check does to the verification: tentatives, unique, RANSAC samples and inliers of the graf ladder and of three pairs with
40 % inliers (bench.py's harder_verification scenes) per mode.
  python tools/mutual_timing.py [reps]                         the report (profiles/mutual_timing.txt)
  python tools/mutual_timing.py [reps] --against OTHER.so      ... and mode 0 of this build against another build of the library (the
                                                               parent commit's), three alternating runs each in fresh processes
  python tools/mutual_timing.py [reps] --pipeline              ... and pairs/s of the benchmark's pipeline shape at modes 0 and 1
  python tools/mutual_timing.py [reps] --mode0 [--lib X.so]    one such run: a JSON line with the three match-stage times"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

INPUTS = ("synthetic 60156 x 47177", "graf1 / graf6 ladder banks", "1080p pair")


def timed(ctx, stages, fn, reps):
    fn()                                     # warm-up: buffers grow here
    ctx.timing_enable(stages); ctx.timing_reset()
    for _ in range(reps):
        out = fn()
    ms = [ctx.timing_read(s)[0] / reps for s in stages]
    ctx.timing_enable([])
    return ms, out


def graf_images():
    import torch
    from PIL import Image
    import orc
    g = [orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", n)).convert("RGB"))) for n in ("graf1.png", "graf6.png")]
    h, w = g[0].shape
    img = torch.from_numpy(np.stack(g)).cuda()
    torch.cuda.synchronize()
    return img, w, h


def make_inputs(pkg, ctx):
    """[(name, query bank, train bank)]: ImgReps of the three inputs"""
    import torch
    import synth
    import test_gpu_guided as tg            # (the scene generator of the guided matcher's timing)
    rng = np.random.default_rng(5)
    q, t = tg.scene(rng, 60156, 47177, tg.H_PROJ, w=1920.0, h=1080.0, noise=2.0)
    rq, rt = pkg.ImgRep(ctx, len(q)), pkg.ImgRep(ctx, len(t))
    rq.append_host(q); rt.append_host(t)
    out = [(INPUTS[0], rq, rt)]
    img, w, h = graf_images()
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
    pkg.ransac_pin_seed(4242)
    pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, pkg.iters_mods_steps(), rep1, rep2, pkg.PairParams.default(), min_matches=1 << 30)
    out.append((INPUTS[1], rep1, rep2))
    a, b, _ = synth.pair(1920, 1080, seed=0)
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    ctx.detect_describe_dev(dev.data_ptr(), 2, 1920, 1080)
    p1, p2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
    p1.append_ctx(0); p2.append_ctx(1)
    out.append((INPUTS[2], p1, p2))
    return out


def new_context(pkg):
    d = pkg.view_ctx_dims(800, 640)
    return pkg.Context(0, max(d[0], 1920), max(d[1], 1080), 2)


def mode0_run(reps, lib):
    """the match stage of the three inputs at mode 0, as a JSON line (any build of the library: the setter is not called)"""
    pkg = ge.load_package()
    if lib:
        pkg.LIB_PATH = os.path.abspath(lib)
    ctx = new_context(pkg)
    res = {}
    for name, rq, rt in make_inputs(pkg, ctx):
        (ms,), out = timed(ctx, ["match"], lambda: pkg.match_reps(ctx, rq, rt), reps)
        res[name] = [ms, len(out[0])]
    print("MODE0 " + json.dumps(res))


def against(reps, other):
    runs = {"this build": [], "other build": []}
    for _ in range(3):
        for who, lib in (("other build", other), ("this build", None)):
            cmd = [sys.executable, os.path.abspath(__file__), str(reps), "--mode0"] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("MODE0 ")]
            if p.returncode or not line:
                raise SystemExit("mode-0 run failed (%s): %s" % (who, p.stderr.decode()[-2000:]))
            runs[who].append(json.loads(line[0][6:]))
    print("mode 0 against the other build of the library (%s), match stage in ms, three alternating runs each in fresh processes:" % other)
    for name in INPUTS:
        a = [r[name][0] for r in runs["other build"]]; b = [r[name][0] for r in runs["this build"]]
        assert len({r[name][1] for r in runs["other build"] + runs["this build"]}) == 1, "the two builds return lists of different lengths"
        print("  %-28s other %s (spread %.3f)   this %s (spread %.3f)   difference of the means %+.3f"
              % (name, " ".join("%.3f" % v for v in a), max(a) - min(a), " ".join("%.3f" % v for v in b), max(b) - min(b),
                 sum(b) / 3 - sum(a) / 3))
    print()


def report(reps):
    import torch
    import synth
    pkg = ge.load_package()
    ctx = new_context(pkg)
    print("mutual check of the FGINN matcher, stage timing (HIP events, mean of %d calls after one warm-up), ratio 0.8, contradDist 10, nn 50" % reps)
    print("match = the whole match stage of mods_match_reps; check = the check's own launches inside it (counter reset, list, sweep);")
    print("forward = accepted queries of the forward search (the sweep's candidates), kept = tentatives after the check")
    print()
    inputs = make_inputs(pkg, ctx)
    for name, rq, rt in inputs:
        print("%s: %d queries x %d trains" % (name, len(rq), len(rt)))
        for mode in (0, 1, 2):
            ctx.set_match_mutual(mode)
            (ms, ms_nn1, ms_chk), out = timed(ctx, ["match", "match_nn1", "match_mutual"], lambda: pkg.match_reps(ctx, rq, rt), reps)
            fwd, kept = ctx.match_mutual_counts()
            print("  mode %d: match %.3f ms (pass 1 %.3f), check %.3f ms, forward %d, kept %d" % (mode, ms, ms_nn1, ms_chk, fwd, kept))
        ctx.set_match_mutual(0)
    print()
    print("the verification with and without the check (seed pinned):")
    img, w, h = graf_images()
    for mode in (0, 1, 2):
        ctx.set_match_mutual(mode)
        rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
        pkg.ransac_pin_seed(4242)
        res, _ = pkg.match_ladder_dev(ctx, img.data_ptr(), w, h, pkg.iters_mods_steps(), rep1, rep2, pkg.PairParams.default(), min_matches=1 << 30)
        print("  graf1 / graf6 ladder, mode %d: %d tentatives, %d unique, %d RANSAC samples, %d inliers"
              % (mode, res.n_tentatives, res.n_unique, res.ransac_samples, res.n_inliers))
        rep1.close(); rep2.close()
    hp = [synth.pair_partial(1920, 1080, seed=2900 + i, frac=0.4) for i in range(3)]
    dev = [torch.from_numpy(np.stack([p[0], p[1]])).cuda() for p in hp]
    torch.cuda.synchronize()
    for mode in (0, 1, 2):
        ctx.set_match_mutual(mode)
        rows = []
        for d in dev:
            pkg.ransac_pin_seed(4242)
            res, _ = pkg.match_pair_dev(ctx, d.data_ptr(), 1920, 1080)
            rows.append("%d tentatives / %d unique / %d samples / %d inliers" % (res.n_tentatives, res.n_unique, res.ransac_samples, res.n_inliers))
        print("  pairs with 40 %% inliers (synth.pair_partial, seeds 2900-2902), mode %d: %s" % (mode, "; ".join(rows)))
    pkg.ransac_pin_seed(-1)
    ctx.set_match_mutual(0)
    print()


def pipeline_run(pkg, mode, n_pairs=768, warm=128):
    """pairs/s of the benchmark's pipeline shape (1080p, 4 GPU workers x 16 pairs per batch, 8 verify workers) on six synthetic pairs
    resident in HBM, under `mode`"""
    import time
    import torch
    import synth
    w, h = 1920, 1080
    dev = [torch.from_numpy(np.stack(synth.pair(w, h, seed=1000 + i)[:2])).cuda() for i in range(6)]
    torch.cuda.synchronize()
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), 4, 8, 16, mutual=mode)
    pending, tent, t0 = 0, 0, 0.0
    for i in range(warm + n_pairs):
        if i == warm:
            while pending:
                pipe.next(); pending -= 1
            t0 = time.perf_counter()
        if pending >= pipe.capacity - 1:
            tent += pipe.next()[0].n_tentatives if i >= warm else 0; pending -= 1
        pipe.submit(dev[i % 6].data_ptr(), i); pending += 1
    while pending:
        tent += pipe.next()[0].n_tentatives; pending -= 1
    dt = time.perf_counter() - t0
    pipe.close()
    return n_pairs / dt, tent / n_pairs


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 10
    if "--mode0" in args:
        return mode0_run(reps, args[args.index("--lib") + 1] if "--lib" in args else None)
    report(reps)
    if "--pipeline" in args:
        pkg = ge.load_package()
        print("the benchmark's pipeline shape (1080p, 4 GPU workers x 16 pairs per batch, 8 verify workers; six synthetic pairs in HBM,")
        print("768 pairs timed after 128), alternating modes:")
        for mode in (0, 1, 0, 1):
            pps, tent = pipeline_run(pkg, mode)
            print("  mode %d: %.1f pairs/s, %.0f tentatives per pair" % (mode, pps, tent))
        print()
    if "--against" in args:
        against(reps, args[args.index("--against") + 1])


if __name__ == "__main__":
    main()
