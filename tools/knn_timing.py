#!/usr/bin/env python3
"""The k-nearest-neighbour search (csrc/knn.hip; mods_match_knn_reps) timed with the context's stage timing - HIP events around the
whole search (pack, sweep, merge) and around the matrix-core sweep alone - mean, minimum and maximum of `reps` calls after one warm-up
call of the same shape, next to the FGINN matcher (mods_match_reps, ratio 0.8) measured in the same run on the same banks:
  - random uint8 descriptor banks of 10 000 x 10 000 regions (a 1080p pair) and 60 156 x 47 177 (the size of the matcher's roofline
    leg), k = 1, 2, 10, 50, 64, trains in random order,
  - the 10 000 x 10 000 banks again with the trains sorted nearest first and farthest first for query 0 (k = 50).
The share of peak is the sweep's 2 * 128 * n_q * n_t integer operations over its time, against the 5 POP/s of the int8 matrix cores;
match_nn1_kernel's, on the same lists, stands beside it.
  python tools/knn_timing.py [reps]                         the report (profiles/knn_timing.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

PEAK_OPS = 5.0e15
KS = (1, 2, 10, 50, 64)


def timed(ctx, stages, fn, reps):
    """per stage (mean, min, max) in ms over `reps` calls, each read on its own, after one warm-up call"""
    fn()                                     # warm-up: buffers grow here, code objects load
    ctx.timing_enable(stages)
    ms = [[] for _ in stages]
    for _ in range(reps):
        ctx.timing_reset()
        out = fn()
        for k, s in enumerate(stages):
            ms[k].append(ctx.timing_read(s)[0])
    ctx.timing_enable([])
    return [(sum(v) / reps, min(v), max(v)) for v in ms], out


def span(t):
    return "%.3f ms (%.3f - %.3f)" % t


def share(n_q, n_t, ms):
    return 100.0 * 2.0 * 128.0 * n_q * n_t / (ms * 1e-3) / PEAK_OPS


def banks(pkg, ctx, q, t):
    rq, rt = pkg.ImgRep(ctx, len(q)), pkg.ImgRep(ctx, len(t))
    rq.append_host(q); rt.append_host(t)
    return rq, rt


def one_shape(pkg, ctx, name, rq, rt, ks, reps):
    n_q, n_t = len(rq), len(rt)
    (ms, ms_nn1), tent = timed(ctx, ["match", "match_nn1"], lambda: pkg.match_reps(ctx, rq, rt, ratio=0.8), reps)
    print("%s: %d queries x %d trains" % (name, n_q, n_t))
    print("  mods_match_reps (ratio 0.8): match %s, match_nn1_kernel %s = %.1f %% of 5 POP/s, %d tentatives"
          % (span(ms), span(ms_nn1), share(n_q, n_t, ms_nn1[0]), len(tent[0])))
    for k in ks:
        (ms_knn, ms_sweep), out = timed(ctx, ["knn", "knn_sweep"], lambda: ctx.match_knn_reps(rq, rt, k), reps)
        grid = pkg.knn_grid(n_q, n_t, k)
        print("  k = %2d: knn %s, knn_sweep_kernel %s = %.1f %% of 5 POP/s, %.1f x match_nn1_kernel; grid %d query blocks x %d splits x %d tiles"
              % (k, span(ms_knn), span(ms_sweep), share(n_q, n_t, ms_sweep[0]), ms_sweep[0] / ms_nn1[0], grid[0], grid[1], grid[2]))
    print()


def main():
    import match_cases as mc
    import match_ref as ref
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 10
    pkg = ge.load_package()
    ctx = pkg.Context(0, 2048, 2048, 1)
    print("k-nearest-neighbour search, stage timing (HIP events; mean (minimum - maximum) of %d calls after one warm-up call per shape and k)" % reps)
    print("knn = the whole search (pack, sweep, merge); knn_sweep_kernel = the matrix-core kernel alone; the matcher's figures are of the")
    print("same run on the same banks")
    print()
    rng = np.random.default_rng(2024)
    q, t = mc.random_regions(10000, rng), mc.random_regions(10000, rng)
    rq, rt = banks(pkg, ctx, q, t)
    one_shape(pkg, ctx, "random banks, trains in random order", rq, rt, KS, reps)
    d0 = ref.sqdist(q["desc"][:1], t["desc"])[0]
    near = np.argsort(d0, kind="stable")
    for name, order in (("trains sorted nearest first for query 0", near), ("trains sorted farthest first for query 0", near[::-1].copy())):
        rt.close()
        rt = pkg.ImgRep(ctx, len(t)); rt.append_host(t[order])
        one_shape(pkg, ctx, "random banks, " + name, rq, rt, (50,), reps)
    rq.close(); rt.close()
    q, t = mc.random_regions(60156, rng), mc.random_regions(47177, rng)
    rq, rt = banks(pkg, ctx, q, t)
    one_shape(pkg, ctx, "random banks, trains in random order", rq, rt, KS, reps)
    rq.close(); rt.close()
    ctx.close()


if __name__ == "__main__":
    main()
