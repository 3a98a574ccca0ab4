#!/usr/bin/env python3
"""Match propagation (mods_propagate_matches_dev; csrc/propagate.hip) measured on an MI355X, every case in a fresh process:
  rate      the synthetic 1080p pair, seeds = its verified frames, at cell 4 and cell 2 (reach 1, radius 5, under the verified H
            within 2 px): rows tried and accepted per round; MODS_STAGE_PROPAGATE (HIP events over every launch of the call: the host
            waits between its scopes are outside it) and the wall time of the call, mean (minimum - maximum) of 5 calls after a
            warm-up call; beside it MODS_STAGE_REFINE of mods_refine_matches_dev on as many rows as the propagation tried (its own
            output rows, repeated), same radius, same process; the transfer error of the propagated rows and of the seeds under the
            generating homography.  The calls go to the library with output arrays made once (the Python wrapper makes fresh ones
            of one row per cell for every call, and touching their pages for the first time is host time that is not the library's).
            Per round: MODS_STAGE_PROPAGATE of calls of 1, 2, .. 8 rounds; a round's time is the difference
  kernels   python tools/propagate_timing.py --kernel-stats DIR appends the share of each kernel of csrc/propagate.hip from the
            kernel statistics a kernel trace of `--one profile` left under DIR (cell 4, 8 rounds, 3 calls, a run of its own)
  graf      graf1 / graf6 (tests/golden), one view: counts per round and the share of the lattice that ends occupied.  There is no
            ground truth for graf in the tree
  default   the default path (tools/lsm_timing.py: mods_match_pair_dev of the 1080p pair, and bench.py), this build against another
            build of the library (the parent commit's, --against) in alternating processes
  python tools/propagate_timing.py [--against PARENT.so] [--skip-bench]     the report (profiles/propagate_timing.txt)
  python tools/propagate_timing.py --one CASE                                one case in this process: a JSON line"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

import lsm_timing as T      # noqa: E402

REPS, ROUNDS = 5, 3


def propagate(ctx, t, w, h, laf, par):
    return ctx.propagate_matches_dev(t.data_ptr(), w, h, w, t.data_ptr() + 4 * w * h, w, h, w, laf, par)


class Call:
    """mods_propagate_matches_dev with output arrays made once for the configuration"""

    def __init__(self, pkg, ctx, t, w, h, laf, par):
        self.pkg, self.ctx, self.par, self.laf = pkg, ctx, par, np.ascontiguousarray(laf, np.float64)
        room = (w // par.cell) * (h // par.cell)
        self.out, self.u6, self.z = np.zeros((room, 14)), np.zeros((room, 6)), np.zeros(room)
        self.rnd, self.parent = np.zeros(room, np.int32), np.zeros(room, np.int32)
        self.stats = np.zeros((par.rounds + 1, 8), np.int32)
        self.tried = np.zeros((h // par.cell, w // par.cell), np.int32)
        self.n, self.trunc, self.room = C.c_int(0), C.c_int(0), room
        self.img = (C.c_void_p(t.data_ptr()), w, h, w, C.c_void_p(t.data_ptr() + 4 * w * h), w, h, w)

    def __call__(self):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.pkg.lib().mods_propagate_matches_dev(self.ctx.h, *self.img, vp(self.laf), len(self.laf), C.byref(self.par), self.room, vp(self.out),
                                                       vp(self.u6), vp(self.z), None, vp(self.rnd), None, vp(self.parent), C.byref(self.n),
                                                       C.byref(self.trunc), None, vp(self.stats), vp(self.tried), None)
        if rc:
            raise SystemExit("mods_propagate_matches_dev: %d" % rc)
        return self.n.value


def timed(ctx, call, reps):
    """(MODS_STAGE_PROPAGATE ms, wall ms) of `reps` calls after a warm-up call"""
    import torch
    call()
    ev, wall = [], []
    ctx.timing_enable(["propagate"])
    for _ in range(reps):
        ctx.timing_reset()
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(ctx.timing_read("propagate")[0])
    ctx.timing_enable([])
    return ev, wall


def one_rate():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = 1920, 1080
    t, H = T.pair_on_device(pkg, w, h, 0)
    ctx = pkg.Context(0, w, h, 2)
    res, laf = T.verified(pkg, ctx, t, w, h)
    out = {"verified": len(laf), "seed_error": [float(T.transfer(H, laf).mean()), float(np.median(T.transfer(H, laf)))], "cells": [], "per_round": []}
    model = dict(model_type=0, model=list(res.H), model_thr=2.0)
    for cell, rounds in ((4, 8), (4, 32), (2, 8), (2, 32)):
        par = pkg.propagate_defaults(cell=cell, rounds=rounds, **model)
        call = Call(pkg, ctx, t, w, h, laf, par)
        ev, wall = timed(ctx, call, REPS)
        n_out = call.n.value
        tried = int(call.stats.sum())
        rows = call.out[np.arange(tried) % max(n_out, 1)] if n_out else laf
        lsm = pkg.lsm_defaults(radius=par.lsm.radius)
        T.refine(ctx, t, w, h, rows, lsm)
        ctx.timing_enable(["refine"])
        rf = []
        for _ in range(REPS):
            ctx.timing_reset()
            T.refine(ctx, t, w, h, rows, lsm)
            rf.append(ctx.timing_read("refine")[0])
        ctx.timing_enable([])
        e = T.transfer(H, call.out[:n_out]) if n_out else np.zeros(1)
        out["cells"].append({"cell": cell, "rounds": rounds, "n_out": n_out, "tried": tried, "stats": call.stats.tolist(),
                             "events": T.stats(ev), "wall": T.stats(wall), "refine": T.stats(rf), "refine_rows": len(rows),
                             "error": [float(e.mean()), float(np.median(e)), float(e.max())],
                             "occupied": float((call.tried == 0).mean())})
    for cell in (4, 2):
        cum = []
        for r in range(1, 9):
            ev, wall = timed(ctx, Call(pkg, ctx, t, w, h, laf, pkg.propagate_defaults(cell=cell, rounds=r, **model)), 3)
            cum.append([float(np.mean(ev)), float(np.mean(wall))])
        out["per_round"].append({"cell": cell, "cumulative": cum})
    print(json.dumps(out))
    ctx.close()


def one_profile():
    """the process to run under a kernel trace: cell 4, 8 rounds, three calls"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = 1920, 1080
    t, H = T.pair_on_device(pkg, w, h, 0)
    ctx = pkg.Context(0, w, h, 2)
    res, laf = T.verified(pkg, ctx, t, w, h)
    call = Call(pkg, ctx, t, w, h, laf, pkg.propagate_defaults(cell=4, rounds=8, model_type=0, model=list(res.H), model_thr=2.0))
    for _ in range(3):
        n = call()
    print(json.dumps({"profiled": 3, "n_out": n}))
    ctx.close()


def kernel_stats(root):
    """appends the kernels of csrc/propagate.hip from a kernel trace to the report: the trace's database (its `kernels` view: name,
    duration in ns per dispatch) or its statistics in CSV form (Name, Calls, TotalDurationNs), whichever the profiler wrote under root"""
    import csv
    import glob
    import sqlite3
    short = lambda name: name.split("(")[0].replace("void ", "").replace("mods::", "")
    rows = []
    for fn in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(fn)):
            if "prop_" in r["Name"]:
                rows.append((short(r["Name"]), int(r["Calls"]), float(r["TotalDurationNs"])))
    if not rows:
        for fn in glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True):
            db = sqlite3.connect(fn)
            for name, calls, ns in db.execute("select name, count(*), sum(duration) from kernels where name like '%prop_%' group by name"):
                rows.append((short(name), int(calls), float(ns)))
    if not rows:
        raise SystemExit("no kernel of csrc/propagate.hip in the statistics under %s" % root)
    total = sum(r[2] for r in rows)
    out = ["kernel trace of three calls (cell 4, 8 rounds, the 1080p pair), a run of its own: the kernels of csrc/propagate.hip, share of their sum (%.3f ms a call)"
           % (total / 3e6)]
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        out.append("  %-28s %5d launches  %8.3f ms a call  %5.1f %%" % (name, calls, ns / 3e6, 100 * ns / total))
    fn = os.path.join(ROOT, "profiles", "propagate_timing.txt")
    open(fn, "a").write("\n".join(out) + "\n")
    print("\n".join(out))


def one_graf():
    import torch
    import __graft_entry__ as ge
    import orc
    from PIL import Image
    pkg = ge.load_package()
    a, b = (orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", fn)).convert("RGB"))) for fn in ("graf1.png", "graf6.png"))
    h, w = a.shape
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
    pkg.ransac_pin_seed(4242)
    res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0, init_sigma=0.2)], rep1, rep2, min_matches=100000,
                                  max_matches=1 << 20)
    pkg.ransac_pin_seed(-1)
    laf = ctx.verified_lafs()
    out = []
    for cell, model in ((4, 0), (4, -1), (2, 0)):
        par = pkg.propagate_defaults(cell=cell, rounds=32, model_type=model, model=list(res.H), model_thr=2.0)
        got = propagate(ctx, t, w, h, laf, par)
        out.append({"cell": cell, "model": model, "seeds": len(laf), "seed_status": np.bincount(got["seed_status"], minlength=8).tolist(),
                    "n_out": len(got["laf"]), "stats": got["stats"].tolist(), "occupied": float((got["tried_status"] == 0).mean()),
                    "zncc": float(got["zncc"].mean()) if len(got["laf"]) else 0.0})
    rep1.close(); rep2.close(); ctx.close()
    print(json.dumps(out))


def spawn(case):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case], capture_output=True, text=True, timeout=500)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{") or l.startswith("[")]
    if p.returncode or not lines:
        raise SystemExit("run of case %s failed:\n%s" % (case, (p.stdout + p.stderr)[-3000:]))
    return json.loads(lines[-1])


def per_round(stats):
    rows = [(sum(r), r[0]) for r in stats]
    last = max([i for i, r in enumerate(rows) if r[0]] + [0])
    return " ".join("%d/%d" % r for r in rows[1:last + 1])


def main():
    args = sys.argv[1:]
    if "--one" in args:
        return {"rate": one_rate, "graf": one_graf, "profile": one_profile}[args[args.index("--one") + 1]]()
    if "--kernel-stats" in args:
        return kernel_stats(args[args.index("--kernel-stats") + 1])
    other = args[args.index("--against") + 1] if "--against" in args else None
    out = ["match propagation (csrc/propagate.hip) on an MI355X; every case in a fresh process", ""]
    r = spawn("rate")
    out.append("synthetic 1080p pair, %d verified frames as seeds (transfer error under the generating homography %.3f mean / %.3f median px);"
               % (r["verified"], *r["seed_error"]))
    out.append("reach 1, radius 5, under the verified H within 2 px; mean (minimum - maximum) of %d calls after a warm-up call" % REPS)
    for c in r["cells"]:
        out.append("  cell %d, %2d rounds: %d rows tried, %d accepted (%.1f %% of the lattice occupied by them); tried/accepted per round: %s"
                   % (c["cell"], c["rounds"], c["tried"], c["n_out"], 100 * c["occupied"], per_round(c["stats"])))
        out.append("      MODS_STAGE_PROPAGATE %s; wall time of the call %s (the difference: host waits, copies, launches)"
                   % (T.span(c["events"]), T.span(c["wall"])))
        out.append("      mods_refine_matches_dev on %d rows, MODS_STAGE_REFINE %s: propagation / refinement = %.2f (events), %.2f (wall / events)"
                   % (c["refine_rows"], T.span(c["refine"]), c["events"]["mean"] / c["refine"]["mean"], c["wall"]["mean"] / c["refine"]["mean"]))
        out.append("      transfer error of the propagated rows: %.3f mean / %.3f median / %.3f max px" % tuple(c["error"]))
    for pr in r["per_round"]:
        cum = pr["cumulative"]
        inc = [cum[0][0]] + [cum[i][0] - cum[i - 1][0] for i in range(1, len(cum))]
        out.append("  cell %d, MODS_STAGE_PROPAGATE of calls of 1 .. 8 rounds (3 calls each): %s ms; per round (round 1 with the seeds): %s ms;"
                   % (pr["cell"], " ".join("%.2f" % c[0] for c in cum), " ".join("%.2f" % v for v in inc)))
        out.append("      wall time of the same calls: %s ms (wall - events = host waits, copies and launches: %s ms)"
                   % (" ".join("%.2f" % c[1] for c in cum), " ".join("%.2f" % (c[1] - c[0]) for c in cum)))
    out.append("")
    out.append("graf1 / graf6 (tests/golden, 800 x 640), one view, RANSAC seed pinned, 32 rounds; no ground truth in the tree: counts and coverage only")
    for g in spawn("graf"):
        out.append("  cell %d, %s: %d seeds (%d OK), %d rows accepted of %d tried, %.1f %% of the lattice; mean zncc %.3f; tried/accepted per round: %s"
                   % (g["cell"], "under the verified H" if g["model"] == 0 else "no model", g["seeds"], g["seed_status"][0], g["n_out"],
                      sum(sum(s) for s in g["stats"][1:]), 100 * g["occupied"], g["zncc"], per_round(g["stats"])))
    out.append("")
    runs = {"this build": [], "parent": []}
    for _ in range(ROUNDS):
        runs["this build"].append(T.spawn("default"))
        if other:
            runs["parent"].append(T.spawn("default", other))
    out.append("default path: mods_match_pair_dev of the 1080p pair (wall time, %d calls per process), %d rounds of fresh processes, alternating" % (T.REPS, ROUNDS))
    for name, rs in runs.items():
        if rs:
            v = [x["pair"]["mean"] for x in rs]
            out.append("  %-11s %s ms   spread (max - min) %.3f" % (name, " ".join("%.3f" % x for x in v), max(v) - min(v)))
    out.append("")
    if "--skip-bench" not in args:
        runs = {"this build": [], "parent": []}
        for _ in range(ROUNDS):
            runs["this build"].append(T.spawn("bench"))
            if other:
                runs["parent"].append(T.spawn("bench", other))
        out.append("bench.py --gpus 1 --steps 10 --warmup 2 (pairs/s), %d rounds of fresh processes, alternating" % ROUNDS)
        for name, rs in runs.items():
            if rs:
                v = [float(x["value"]) for x in rs]
                out.append("  %-11s %s   spread (max - min) %.4g" % (name, " ".join("%.5g" % x for x in v), max(v) - min(v)))
        out.append("")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "propagate_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
