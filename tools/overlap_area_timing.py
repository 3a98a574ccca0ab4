#!/usr/bin/env python3
"""Area-overlap matching (csrc/overlap_area.hip) timed with the context's stage timing (HIP events around the two scopes of a search:
pack, both gate sweeps, the lattice walk, accept, compaction, emit; the host's wait between the scopes is not in it), next to the
linearised search of csrc/overlap.hip on the same banks in the same run:
  - the scene of tests/overlap_ref.py with 5000 x 4099 regions in its 400 x 300 frame;
  - a dense case, 12000 x 12000 regions in a 640 x 480 frame.
The evaluated pairs and their lattice points are counted by the numpy restatement of the gates (tests/overlap_area_ref.py), so the
rates are what the contract asks for over the stage time, not what a kernel counted about itself.  Writes the profile text
(profiles/overlap_area_timing.txt).  python tools/overlap_area_timing.py [reps] [out]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import overlap_area_ref as oar  # noqa: E402  (the gates, for the work counts)
import overlap_ref as orf  # noqa: E402  (the scene generator)


def work(q, t, p):
    """(evaluated pairs, lattice points) of the lists by the contract's gates"""
    mq, mt = orf.common_masks(q, t, p)
    tr = tuple(a[None, :] for a in oar.train_records(t))
    qr = orf.query_records(q, list(p.H))
    pairs = points = 0
    for q0 in range(0, len(q), orf.CHUNK):
        q1 = min(len(q), q0 + orf.CHUNK)
        s = oar._setup(tuple(a[q0:q1, None] for a in qr), tr, p.max_error)
        ev = s.ev & mq[q0:q1, None] & mt[None, :]
        x0, x1, y0, y1 = (m[ev] for m in s.box)
        pairs += int(ev.sum())
        points += int(((x1 - x0 + 1.0) * (y1 - y0 + 1.0)).sum())
    return pairs, points


def timed(ctx, stage, fn, reps):
    fn()                                     # warm-up: buffers grow here
    ctx.timing_enable([stage]); ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    ms, n, _ = ctx.timing_read(stage)
    ctx.timing_enable([])
    return ms / reps, wall, out


def case(pkg, ctx, say, name, n_q, n_t, w, h, seed, reps):
    q, t = orf.scene(np.random.default_rng(seed), n_q, n_t, orf.H_PROJ, w=float(w), h=float(h))
    rq, rt = pkg.ImgRep(ctx, len(q)), pkg.ImgRep(ctx, len(t))
    rq.append_host(q); rt.append_host(t)
    size = dict(w1=w, h1=h, w2=w, h2=h)
    pairs, points = work(q, t, oar.params(orf.H_PROJ, 0.4, 2, **size))
    say("%s: %d x %d regions in %d x %d, %d evaluated pairs (%.2f %% of all), %d lattice points (%.0f per pair)"
        % (name, n_q, n_t, w, h, pairs, 100.0 * pairs / (n_q * n_t), points, points / max(pairs, 1)))
    for mode in (2, 1, 0):
        p = pkg.OverlapAreaParams.default(orf.H_PROJ, max_error=0.4, one_to_one=mode, **size)
        ms, wall, (m, c) = timed(ctx, "overlap_area", lambda: pkg.match_overlap_area_reps(ctx, rq, rt, p), reps)
        say("  area, one_to_one %d: overlap_area %.3f ms (call %.3f ms on the host's clock), %.1f M evaluated pairs/s, %.2f G lattice points/s; "
            "%d matches, common area %d | %d, repeatability %.4f"
            % (mode, ms, wall, pairs / ms / 1e3, points / ms / 1e6, c.n_matches, c.n_q_common, c.n_t_common, c.repeatability))
    for one in (1, 0):
        p = pkg.OverlapParams.default(orf.H_PROJ, max_error=0.09, oriented=1, one_to_one=one, **size)
        ms, wall, (m, c) = timed(ctx, "overlap", lambda: pkg.match_overlap_reps(ctx, rq, rt, p), reps)
        say("  linearised (E < 0.09, oriented), one_to_one %d: overlap %.3f ms (call %.3f ms), %d matches, repeatability %.4f"
            % (one, ms, wall, c.n_matches, c.repeatability))
    p = pkg.OverlapAreaParams.default(orf.H_PROJ, max_error=0.4, one_to_one=2, **size)
    try:
        for splits in (1, 4, 16):
            ctx.overlap_splits(splits)
            ms, _, _ = timed(ctx, "overlap_area", lambda: pkg.match_overlap_area_reps(ctx, rq, rt, p), reps)
            say("  area, one_to_one 2 with %2d train split(s) of the gate sweeps: overlap_area %.3f ms" % (splits, ms))
    finally:
        ctx.overlap_splits(0)
    rq.close(); rt.close()
    say("")


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "overlap_area_timing.txt")
    pkg = ge.load_package()
    ctx = pkg.Context(0, 1920, 1080, 2)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say("area-overlap matching, stage timing (HIP events, mean of %d calls after one warm-up; MI355X); overlap = the linearised search of" % reps)
    say("mods_match_overlap_reps on the same banks in the same run.  Pairs and lattice points: counted by the numpy gates of the contract")
    say("")
    case(pkg, ctx, say, "scene", 5000, 4099, 400, 300, 5, reps)
    case(pkg, ctx, say, "dense", 12000, 12000, 640, 480, 6, reps)
    ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
