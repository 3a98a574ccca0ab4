#!/usr/bin/env python3
"""The least-squares refinement of correspondences (mods_refine_matches_dev; csrc/refine.hip) measured on an MI355X, every case in a
fresh process:
  stage     MODS_STAGE_REFINE (HIP events) for 3 000 and 20 000 correspondences on a synthetic 1080p pair at radius 5 / 10 / 15: the
            verified frames of the pair, drawn with replacement and moved by up to 1 px so that every row iterates; mean (minimum -
            maximum) of 5 calls after a warm-up call
  default   the default path, mods_match_pair_dev of the same pair (wall time around the call, the stream waited for), this build
            against another build of the library (the parent commit's, --against) in alternating processes
  bench     bench.py --gpus 1 --steps 10 --warmup 2, unchanged, alternating the two builds
  synth     the synthetic pairs with their generating homography: transfer error of the verified matches before and after, and the
            corner error of the verified H against the refit H
  graf      graf1 / graf6 (tests/golden), one view and the ladder: count per status, mean zncc before and after, and the RMS residual
            of the matches under their own least-squares homography before and after.  There is no ground truth for graf here
  python tools/lsm_timing.py [--against PARENT.so] [--skip-bench]     the report (profiles/lsm_timing.txt)
  python tools/lsm_timing.py --one CASE                one case in this process: a JSON line
  python tools/lsm_timing.py --profile                 20 000 rows at radius 10, three calls (the process to run under a profiler)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, ROUNDS = 5, 3
COUNTS, RADII = (3000, 20000), (5, 10, 15)
STATUS = ("ok", "maxiter", "bad frame", "outside", "flat", "diverged", "low zncc")


def stats(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v))}


def span(s):
    return "%.3f ms (%.3f - %.3f)" % (s["mean"], s["min"], s["max"])


def pair_on_device(pkg, w, h, seed):
    import torch
    import synth
    a, b, H = synth.pair(w, h, seed=seed)
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    return t, H


def verified(pkg, ctx, t, w, h, seed=4242):
    pkg.ransac_pin_seed(seed)
    res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=1 << 20)
    pkg.ransac_pin_seed(-1)
    return res, ctx.verified_lafs()


def refine(ctx, t, w, h, laf, par=None):
    return ctx.refine_matches_dev(t.data_ptr(), w, h, w, t.data_ptr() + 4 * w * h, w, h, w, laf, par)


def rows_of(laf, n, seed):
    """n rows drawn from the verified frames, the second centre moved by up to 1 px"""
    rng = np.random.default_rng(seed)
    out = laf[rng.integers(0, len(laf), n)].copy()
    ang, rad = rng.uniform(0, 2 * np.pi, n), np.sqrt(rng.uniform(0, 1, n))
    out[:, 7] += rad * np.cos(ang); out[:, 8] += rad * np.sin(ang)
    return out


def one_stage():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = 1920, 1080
    t, _ = pair_on_device(pkg, w, h, 0)
    ctx = pkg.Context(0, w, h, 2)
    res, laf = verified(pkg, ctx, t, w, h)
    out = {"verified": len(laf), "rows": []}
    for n in COUNTS:
        rows = rows_of(laf, n, n)
        for R in RADII:
            par = pkg.lsm_defaults(radius=R)
            got = refine(ctx, t, w, h, rows, par)          # warm-up: the buffer grows here
            ctx.timing_enable(["refine"])
            ms = []
            for _ in range(REPS):
                ctx.timing_reset()
                refine(ctx, t, w, h, rows, par)
                ms.append(ctx.timing_read("refine")[0])
            ctx.timing_enable([])
            out["rows"].append({"n": n, "radius": R, "ms": stats(ms), "iterations": float(got["iterations"].mean()),
                                "status": np.bincount(got["status"], minlength=7).tolist()})
    print(json.dumps(out))
    ctx.close()


def one_default():
    """(only calls that the parent's library has as well)"""
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = 1920, 1080
    t, _ = pair_on_device(pkg, w, h, 0)
    ctx = pkg.Context(0, w, h, 2)
    pkg.ransac_pin_seed(4242)
    pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=1 << 20)
    ms = []
    for _ in range(REPS):
        pkg.ransac_pin_seed(4242)
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.perf_counter()
        res, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=1 << 20)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    pkg.ransac_pin_seed(-1)
    print(json.dumps({"pair": stats(ms), "inliers": res.n_inliers}))
    ctx.close()


def one_bench():
    """bench.py in this process, unchanged"""
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"]
    bench.main()


def transfer(H, laf):
    p = np.c_[laf[:, 0:2], np.ones(len(laf))] @ np.asarray(H, np.float64).reshape(3, 3).T
    return np.hypot(*(p[:, :2] / p[:, 2:] - laf[:, 7:9]).T)


def corner_error(H, H_true, w, h):
    c = np.array([[0.0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]])
    p, q = c @ np.asarray(H, np.float64).reshape(3, 3).T, c @ np.asarray(H_true, np.float64).reshape(3, 3).T
    return float(np.hypot(*(p[:, :2] / p[:, 2:] - q[:, :2] / q[:, 2:]).T).mean())


def one_synth():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    out = []
    for (w, h, seed) in ((400, 300, 7), (800, 600, 3), (1920, 1080, 0)):
        t, H = pair_on_device(pkg, w, h, seed)
        ctx = pkg.Context(0, w, h, 2)
        res, laf = verified(pkg, ctx, t, w, h)
        for R in (5, 10):
            got = refine(ctx, t, w, h, laf, pkg.lsm_defaults(radius=R))
            acc = got["status"] <= 1
            e0, e1 = transfer(H, laf), transfer(H, got["laf"])
            out.append({"w": w, "h": h, "radius": R, "n": len(laf), "status": np.bincount(got["status"], minlength=7).tolist(),
                        "before": [float(e0.mean()), float(np.median(e0))], "after": [float(e1.mean()), float(np.median(e1))],
                        "zncc": [float(got["zncc_before"][acc].mean()), float(got["zncc_after"][acc].mean())],
                        "iterations": float(got["iterations"][acc].mean()),
                        "corner": [corner_error(list(res.H), H, w, h), corner_error(pkg.refit_model(pkg_u6(laf), 0), H, w, h),
                                   corner_error(pkg.refit_model(got["u6"], 0), H, w, h)]})
        ctx.close()
    print(json.dumps(out))


def pkg_u6(laf):
    one = np.ones(len(laf))
    return np.stack([laf[:, 0], laf[:, 1], one, laf[:, 7], laf[:, 8], one], axis=1)


def rms_under_own_model(pkg, u6):
    if len(u6) < 4:
        return float("nan")
    H = pkg.refit_model(u6, 0)
    laf = np.zeros((len(u6), 14)); laf[:, 0:2] = u6[:, 0:2]; laf[:, 7:9] = u6[:, 3:5]
    return float(np.sqrt(np.mean(transfer(H, laf) ** 2)))


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
    out = []
    ladders = {"one view": [pkg.LadderStep.make((1,), 360.0, init_sigma=0.2)],
               "ladder": [pkg.LadderStep.make((1,), 360.0, init_sigma=0.2), pkg.LadderStep.make((1, 5, 9), 360.0 / 2.5, init_sigma=0.2)]}
    for name, steps in ladders.items():
        ctx = pkg.Context(0, d[0], d[1], 1)
        rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
        pkg.ransac_pin_seed(4242)
        res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep1, rep2, min_matches=100000, max_matches=1 << 20)
        pkg.ransac_pin_seed(-1)
        laf = ctx.verified_lafs()
        for R in (5, 10):
            got = refine(ctx, t, w, h, laf, pkg.lsm_defaults(radius=R))
            acc = got["status"] <= 1
            out.append({"name": name, "radius": R, "n": len(laf), "status": np.bincount(got["status"], minlength=7).tolist(),
                        "zncc": [float(got["zncc_before"][acc].mean()) if acc.any() else 0.0, float(got["zncc_after"][acc].mean()) if acc.any() else 0.0],
                        "rms_all": [rms_under_own_model(pkg, pkg_u6(laf)), rms_under_own_model(pkg, got["u6"])],
                        "rms_accepted": [rms_under_own_model(pkg, pkg_u6(laf[acc])), rms_under_own_model(pkg, got["u6"][acc])]})
        rep1.close(); rep2.close(); ctx.close()
    print(json.dumps(out))


def profile_run():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = 1920, 1080
    t, _ = pair_on_device(pkg, w, h, 0)
    ctx = pkg.Context(0, w, h, 2)
    res, laf = verified(pkg, ctx, t, w, h)
    rows = rows_of(laf, 20000, 20000)
    for _ in range(3):
        got = refine(ctx, t, w, h, rows, pkg.lsm_defaults(radius=10))
    print("profiled: 3 calls, 20000 rows, radius 10, %.2f iterations per row" % got["iterations"].mean())
    ctx.close()


def spawn(case, lib=None):
    env = dict(os.environ)
    if lib:
        env["MODS_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case], env=env, capture_output=True, text=True, timeout=500)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{") or l.startswith("[")]
    if p.returncode or not lines:
        raise SystemExit("run of case %s failed:\n%s" % (case, (p.stdout + p.stderr)[-3000:]))
    return json.loads(lines[-1])


def counts(st):
    return ", ".join("%d %s" % (c, n) for c, n in zip(st, STATUS) if c)


def main():
    args = sys.argv[1:]
    if "--profile" in args:
        return profile_run()
    if "--one" in args:
        return {"stage": one_stage, "default": one_default, "bench": one_bench, "synth": one_synth, "graf": one_graf}[args[args.index("--one") + 1]]()
    other = args[args.index("--against") + 1] if "--against" in args else None
    out = ["least-squares refinement of correspondences (csrc/refine.hip) on an MI355X; every case in a fresh process", ""]
    r = spawn("stage")
    out.append("MODS_STAGE_REFINE (HIP events), synthetic 1080p pair, rows drawn from its %d verified frames and moved by up to 1 px;" % r["verified"])
    out.append("mean (minimum - maximum) of %d calls after a warm-up call" % REPS)
    for row in r["rows"]:
        out.append("  %5d rows, radius %2d: %s = %.2f us per row, %.2f iterations per row; %s"
                   % (row["n"], row["radius"], span(row["ms"]), 1e3 * row["ms"]["mean"] / row["n"], row["iterations"], counts(row["status"])))
    out.append("")
    runs = {"this build": [], "parent": []}
    for _ in range(ROUNDS):
        runs["this build"].append(spawn("default"))
        if other:
            runs["parent"].append(spawn("default", other))
    out.append("default path: mods_match_pair_dev of the same pair (wall time, %d calls per process), %d rounds of fresh processes, alternating" % (REPS, ROUNDS))
    for name, rs in runs.items():
        if rs:
            v = [x["pair"]["mean"] for x in rs]
            out.append("  %-11s %s ms   spread (max - min) %.3f" % (name, " ".join("%.3f" % x for x in v), max(v) - min(v)))
    out.append("")
    if "--skip-bench" not in args:
        runs = {"this build": [], "parent": []}
        for _ in range(ROUNDS):
            runs["this build"].append(spawn("bench"))
            if other:
                runs["parent"].append(spawn("bench", other))
        out.append("bench.py --gpus 1 --steps 10 --warmup 2 (pairs/s), %d rounds of fresh processes, alternating" % ROUNDS)
        for name, rs in runs.items():
            if rs:
                v = [float(x["value"]) for x in rs]
                out.append("  %-11s %s   spread (max - min) %.4g" % (name, " ".join("%.5g" % x for x in v), max(v) - min(v)))
        out.append("")
    out.append("synthetic pairs (tests/synth.py: sigma = 2 noise, rounded to 8 bits) against their generating homography, verified matches of")
    out.append("mods_match_pair_dev: transfer error |H_true x1 - x2| in px as mean / median; corner error (mean of the four image corners)")
    for row in spawn("synth"):
        out.append("  %4d x %4d, radius %2d: %d rows (%s); before %.3f / %.3f, after %.3f / %.3f; zncc %.3f -> %.3f; %.2f iterations"
                   % (row["w"], row["h"], row["radius"], row["n"], counts(row["status"]), *row["before"], *row["after"], *row["zncc"], row["iterations"]))
        out.append("      corner error: verified H %.3f, least-squares H of the unrefined rows %.3f, of the refined rows %.3f" % tuple(row["corner"]))
    out.append("")
    out.append("graf1 / graf6 (tests/golden, 800 x 640), RANSAC seed pinned; RMS residual of the matches under their own least-squares")
    out.append("homography (mods_refit_model), before -> after.  There is no ground-truth homography for graf in the tree: no accuracy is claimed")
    for row in spawn("graf"):
        out.append("  %-8s radius %2d: %d rows: %s; zncc of the accepted %.3f -> %.3f; RMS all rows %.3f -> %.3f px, accepted rows %.3f -> %.3f px"
                   % (row["name"], row["radius"], row["n"], counts(row["status"]), *row["zncc"], *row["rms_all"], *row["rms_accepted"]))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "lsm_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
