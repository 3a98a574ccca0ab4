#!/usr/bin/env python3
"""Domain-size pooling of the SIFT descriptor (mods_ctx_domain_pooling; csrc/sift.hip: sift_wave2_kernel<.., true>, dsp_finish_kernel) timed
with the context's stage timing - HIP events around the extraction and the SIFT launches of a detect + describe call - on the
benchmark's shape, a batch of 16 synthetic 1920 x 1080 images: pooling off and K = 2, 3, 5 domains, alternating, `rounds` rounds of
`reps` calls each after one warm-up call per setting.  The yardstick of K domains is K times the unpooled EXTRACT + SIFT time.
Then what pooling does to graf1 / graf6 (tests/golden; one identity view, H verification, default parameters, seed pinned).
  python tools/dsp_timing.py [reps]                       the report, also written to profiles/dsp_timing.txt
  python tools/dsp_timing.py [reps] --against OTHER.so    ... and the unpooled call of this build against another build of the library
                                                          (the parent commit's), three alternating runs each in fresh processes
  python tools/dsp_timing.py [reps] --off [--lib X.so]    one such run: a JSON line with the unpooled stage times"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

W, H, N_IMG = 1920, 1080, 16
STAGES = ["describe", "extract", "sift"]
SETTINGS = [(0, 0.0, 0.0), (2, 0.5, 1.5), (3, 0.5, 1.5), (5, 0.5, 2.0)]
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def batch():
    import torch
    import synth
    imgs = []
    for i in range(N_IMG // 2):
        a, b, _ = synth.pair(W, H, seed=1000 + i)
        imgs += [a, b]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    torch.cuda.synchronize()
    return t


def timed(ctx, fn, reps):
    fn()                                     # warm-up: buffers grow here
    ctx.timing_enable(STAGES); ctx.timing_reset()
    for _ in range(reps):
        fn()
    ms = [ctx.timing_read(s)[0] / reps for s in STAGES]
    ctx.timing_enable([])
    return ms


def off_run(reps, lib):
    """the unpooled call as a JSON line (any build of the library: the setter is not called)"""
    pkg = ge.load_package()
    if lib:
        pkg.LIB_PATH = os.path.abspath(lib)
    ctx = pkg.Context(0, W, H, N_IMG)
    t = batch()
    ms = timed(ctx, lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H), reps)
    n = sum(len(ctx.regions_fetch(i)) for i in range(N_IMG))
    print("OFF " + json.dumps({"ms": ms, "regions": n}))


def against(reps, other):
    runs = {"other build": [], "this build": []}
    for _ in range(3):
        for who, lib in (("other build", other), ("this build", None)):
            cmd = [sys.executable, os.path.abspath(__file__), str(reps), "--off"] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("OFF ")]
            if p.returncode or not line:
                raise SystemExit("unpooled run failed (%s): %s" % (who, p.stderr.decode()[-2000:]))
            runs[who].append(json.loads(line[0][4:]))
    assert len({r["regions"] for rr in runs.values() for r in rr}) == 1, "the two builds describe different numbers of regions"
    say("pooling off against the other build of the library (%s), EXTRACT + SIFT in ms, three alternating runs each in fresh processes:" % other)
    mean = {}
    for who in ("other build", "this build"):
        v = [r["ms"][1] + r["ms"][2] for r in runs[who]]
        mean[who] = sum(v) / 3
        say("  %-12s %s (spread %.3f)" % (who, " ".join("%.3f" % x for x in v), max(v) - min(v)))
    say("  difference of the means %+.3f ms" % (mean["this build"] - mean["other build"]))
    say()
    return mean["other build"]


def report(reps, rounds=3):
    pkg = ge.load_package()
    ctx = pkg.Context(0, W, H, N_IMG)
    t = batch()
    say("domain-size pooling, stage timing (HIP events) of detect + describe on %d synthetic %d x %d images (synth.pair, seeds 1000-%d)," % (N_IMG, W, H, 1000 + N_IMG // 2 - 1))
    say("%d rounds, the settings alternating inside a round, mean of %d calls after one warm-up call per setting" % (rounds, reps))
    rows = {s: [] for s in SETTINGS}
    n_regions = 0
    for _ in range(rounds):
        for s in SETTINGS:
            ctx.set_domain_pooling(*s)
            rows[s].append(timed(ctx, lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H), reps))
            n_regions = sum(len(ctx.regions_fetch(i)) for i in range(N_IMG))
    ctx.set_domain_pooling(0)
    say("regions of the batch: %d" % n_regions)
    say()
    mean = {s: [sum(r[j] for r in rows[s]) / rounds for j in range(3)] for s in SETTINGS}
    off = mean[SETTINGS[0]][1] + mean[SETTINGS[0]][2]
    for s in SETTINGS:
        es = [r[1] + r[2] for r in rows[s]]
        name = "off" if s[0] == 0 else "K = %d (%g .. %g)" % s
        line = "  %-18s EXTRACT %.3f ms  SIFT %.3f ms  EXTRACT + SIFT %.3f ms (rounds: %s; spread %.3f)  DESCRIBE stage %.3f ms" % (
            name, mean[s][1], mean[s][2], sum(es) / rounds, " ".join("%.3f" % v for v in es), max(es) - min(es), mean[s][0])
        if s[0]:
            line += "  = %.2f x the yardstick (K x off = %.3f ms)" % ((sum(es) / rounds) / (s[0] * off), s[0] * off)
        say(line)
    say("  (SIFT with pooling on: K x the pooled form of sift_wave2_kernel + dsp_finish_kernel; off: sift_wave2_kernel)")
    say()
    ctx.close()
    return off


def graf(pkg):
    import torch
    from PIL import Image
    import orc
    g = [orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", n)).convert("RGB"))) for n in ("graf1.png", "graf6.png")]
    h, w = g[0].shape
    img = torch.from_numpy(np.stack(g)).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    say("graf1 / graf6 (%d x %d), mods_match_pair_dev: one identity view per image, H verification, default parameters, RANSAC seed 4242:" % (w, h))
    for s in ((0, 0.0, 0.0), (3, 0.5, 1.5), (5, 0.5, 2.0)):
        ctx.set_domain_pooling(*s)
        pkg.ransac_pin_seed(4242)
        res, _ = pkg.match_pair_dev(ctx, img.data_ptr(), w, h)
        say("  %-18s regions %d | %d, tentatives %d, unique %d, verified inliers %d (RANSAC samples %d)"
            % ("off" if s[0] == 0 else "K = %d (%g .. %g)" % s, res.n_described[0], res.n_described[1], res.n_tentatives, res.n_unique,
               res.n_inliers, res.ransac_samples))
    pkg.ransac_pin_seed(-1)
    ctx.close()
    say()


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 10
    if "--off" in args:
        return off_run(reps, args[args.index("--lib") + 1] if "--lib" in args else None)
    pkg = ge.load_package()
    if pkg.lib().mods_device_count() <= 0:
        raise SystemExit("no HIP device: the timing needs the GPU")
    report(reps)
    graf(pkg)
    if "--against" in args:
        against(reps, args[args.index("--against") + 1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dsp_timing.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
