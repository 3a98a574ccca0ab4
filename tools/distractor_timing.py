#!/usr/bin/env python3
"""The distractor database of the FGINN ratio test (mods_descdb_*, mods_ctx_distractor_db; csrc/distractor.hip) measured on an MI355X,
every case in a fresh process:
  sweep    mods_descdb_min_dist of 3 000 and 20 000 random queries against random databases of 2^17, 2^20 and 2^22 rows: the stage
           timers DISTRACTOR (pack + sweep) and DISTRACTOR_SWEEP (the matrix-core kernel alone), HIP events, as TOP/s and as a share
           of the 5 POP/s of the int8 matrix cores; match_nn1_kernel on 60 156 x 47 177 random lists from the same process beside it
  match    the match stage (MODS_STAGE_MATCH, HIP events) of a synthetic 1080p pair with no database attached, this build against
           another build of the library (the parent commit's, --against) in alternating processes; the DISTRACTOR timer must count
           no scope
  bench    bench.py --gpus 1 --steps 10 --warmup 2, alternating the two builds; then once more with a 2^20-row random database attached
           to the benchmark's pipeline (bench.py is run unchanged: its Pipeline class is wrapped)
  graf     graf1 / graf6 (tests/golden) through mods_match_pair_dev, one view, homography, ratio 0.8, RANSAC seed pinned, at the
           default configuration and at FixedRegNumber 500 / 1000 / 2000, without and with a database: tentatives, true ones (within
           err_threshold of the homography the default run without a database verified, mods_hmatrix_filter), verified, RANSAC samples.
           The database is the project's own synthetic textures (tests/synth.py) described by the library at several sizes - no
           corpus of natural-image descriptors is at hand
  python tools/distractor_timing.py [reps] [--against PARENT.so] [--skip-bench]     the report (profiles/distractor_timing.txt)
  python tools/distractor_timing.py [reps] --one CASE                                one case in this process: a JSON line"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_OPS = 5.0e15
ROUNDS = 3
QUERIES, ROWS = (3000, 20000), (1 << 17, 1 << 20, 1 << 22)
GRAF_KEEPS = (0, 500, 1000, 2000)
TEXTURES = ((640, 480), (1024, 768), (1600, 1200), (1920, 1080))


def random_rows(n, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((n, 128), np.uint8)
    for b in range(0, n, 1 << 18):
        out[b:b + (1 << 18)] = rng.integers(0, 256, (min(1 << 18, n - b), 128), dtype=np.uint8)
    return out


def stats(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v))}


def one_sweep(reps):
    import __graft_entry__ as ge
    import match_cases as mc
    pkg = ge.load_package()
    ctx = pkg.Context(0, 2048, 2048, 1)
    rows = []
    queries = random_rows(max(QUERIES), 1)
    for m in ROWS:
        db = pkg.DescDB(random_rows(m, 2 + m % 7))
        for n in QUERIES:
            q = queries[:n]
            db.min_dist(ctx, q)                  # warm-up: buffers grow here
            ctx.timing_enable(["distractor", "distractor_sweep"])
            ms = {"distractor": [], "distractor_sweep": []}
            for _ in range(reps):
                ctx.timing_reset()
                db.min_dist(ctx, q)
                for s in ms:
                    ms[s].append(ctx.timing_read(s)[0])
            ctx.timing_enable([])
            rows.append({"m": m, "n": n, "grid": list(pkg.descdb_grid(m, n)), "whole": stats(ms["distractor"]), "sweep": stats(ms["distractor_sweep"])})
        db.close()
    rng = np.random.default_rng(2024)
    rq, rt = pkg.ImgRep(ctx, 60156), pkg.ImgRep(ctx, 47177)
    rq.append_host(mc.random_regions(60156, rng)); rt.append_host(mc.random_regions(47177, rng))
    pkg.match_reps(ctx, rq, rt)
    ctx.timing_enable(["match_nn1"])
    nn1 = []
    for _ in range(reps):
        ctx.timing_reset()
        pkg.match_reps(ctx, rq, rt)
        nn1.append(ctx.timing_read("match_nn1")[0])
    print(json.dumps({"rows": rows, "nn1": stats(nn1)}))
    ctx.close()


def one_match(reps):
    """(only calls that the parent's library has as well)"""
    import torch
    import __graft_entry__ as ge
    import synth
    pkg = ge.load_package()
    w, h = 1920, 1080
    a, b, _ = synth.pair(w, h)
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    nd, nr = ctx.detect_describe_dev(t.data_ptr(), 2, w, h)
    ctx.match_dev(0, 1)
    has = hasattr(pkg.lib(), "mods_ctx_distractor_db")
    ctx.timing_enable(["match"] + (["distractor"] if has else []))
    ms = []
    for _ in range(reps):
        ctx.timing_reset()
        tent, _ = ctx.match_dev(0, 1)
        ms.append(ctx.timing_read("match")[0])
    scopes = ctx.timing_read("distractor")[1] if has else 0
    print(json.dumps({"match": stats(ms), "regions": [int(x) for x in nr], "tentatives": len(tent), "distractor_scopes": scopes}))
    ctx.close()


def one_bench(with_db):
    """bench.py in this process, unchanged; with_db: every Pipeline it makes gets a 2^20-row random database"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if with_db:
        db = pkg.DescDB(random_rows(1 << 20, 9))
        base = pkg.Pipeline

        class WithDb(base):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.set_distractor_db(db)
        pkg.Pipeline = WithDb
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"]
    bench.main()


def texture_rows(pkg):
    """the synthetic textures described by the library: the database of the graf runs"""
    import torch
    import synth
    out = []
    for k, (w, h) in enumerate(TEXTURES):
        ctx = pkg.Context(0, w, h, 2)
        imgs = np.stack([synth.texture(w, h, seed=100 + 2 * k), synth.texture(w, h, seed=101 + 2 * k)]).astype(np.float32)
        t = torch.from_numpy(imgs).cuda()
        torch.cuda.synchronize()
        ctx.detect_describe_dev(t.data_ptr(), 2, w, h)
        out += [ctx.regions_fetch(0)["desc"], ctx.regions_fetch(1)["desc"]]
        ctx.close()
    return np.ascontiguousarray(np.concatenate(out))


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
    rows_db = texture_rows(pkg)
    db = pkg.DescDB(rows_db)
    ctx = pkg.Context(0, w, h, 2)
    rows, h_ref = [], None
    for keep in GRAF_KEEPS:
        par = pkg.PairParams.default()
        if keep:
            par.det.mode, par.det.regionsNumber = 2, keep
        for on in (0, 1):
            ctx.set_distractor_db(db if on else None, None)
            pkg.ransac_pin_seed(4242)
            res, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par)
            if h_ref is None:
                h_ref = np.array(res.H, np.float64).reshape(3, 3)      # the default run without a database
            tent, u6 = ctx.match_dev(0, 1, par.fginn_ratio, par.contradDist, par.nn)
            true = int(pkg.hmatrix_filter(u6, h_ref)[1]) if len(u6) else 0
            rows.append({"keep": keep, "on": on, "described": list(res.n_described), "tentatives": res.n_tentatives, "true": true,
                         "unique": res.n_unique, "inliers": res.n_inliers, "samples": res.ransac_samples})
    pkg.ransac_pin_seed(-1)
    print(json.dumps({"rows": rows, "db_rows": len(rows_db)}))
    ctx.close()


def spawn(case, reps, lib=None, last_json=True):
    env = dict(os.environ)
    if lib:
        env["MODS_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--one", case], env=env, capture_output=True, text=True, timeout=1100)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode or not lines:
        raise SystemExit("run of case %s failed:\n%s" % (case, (p.stdout + p.stderr)[-3000:]))
    return json.loads(lines[-1])


def span(s):
    return "%.3f ms (%.3f - %.3f)" % (s["mean"], s["min"], s["max"])


def bench_figure(out):
    """the headline figure of a bench.py result line, and its name"""
    for key in ("pairs_per_s", "pairs_per_second", "throughput", "value"):
        if key in out and isinstance(out[key], (int, float)):
            return key, float(out[key])
    for key, v in out.items():
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            return key, float(v)
    raise SystemExit("no figure in the bench.py line")


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 10
    if "--one" in args:
        case = args[args.index("--one") + 1]
        return {"sweep": lambda: one_sweep(reps), "match": lambda: one_match(reps), "bench": lambda: one_bench(False),
                "bench_db": lambda: one_bench(True), "graf": one_graf}[case]()
    other = args[args.index("--against") + 1] if "--against" in args else None
    out = ["distractor database (csrc/distractor.hip) on an MI355X; HIP events of the context's stage timers, mean (minimum - maximum) of %d calls" % reps,
           "after a warm-up call; every case in a fresh process", ""]
    r = spawn("sweep", reps)
    out.append("mods_descdb_min_dist, random queries against random databases: DISTRACTOR = pack + sweep, SWEEP = descdb_sweep_kernel alone")
    for row in r["rows"]:
        ops = 2.0 * 128.0 * row["n"] * row["m"]
        tops = ops / (row["sweep"]["mean"] * 1e-3) / 1e12
        out.append("  %5d queries x 2^%d rows: DISTRACTOR %s, SWEEP %s = %.1f TOP/s = %.1f %% of 5 POP/s; grid %d query blocks x %d splits x %d tiles"
                   % (row["n"], int(np.log2(row["m"])), span(row["whole"]), span(row["sweep"]), tops, 100.0 * tops * 1e12 / PEAK_OPS, *row["grid"]))
    nn1 = r["nn1"]
    out.append("  the yardstick, same process: match_nn1_kernel on 60 156 x 47 177 random lists %s = %.1f %% of 5 POP/s"
               % (span(nn1), 100.0 * 2.0 * 128.0 * 60156 * 47177 / (nn1["mean"] * 1e-3) / PEAK_OPS))
    out.append("")
    runs = {"this build": [], "parent": []}
    for _ in range(ROUNDS):
        runs["this build"].append(spawn("match", reps))
        if other:
            runs["parent"].append(spawn("match", reps, other))
    out.append("match stage of a synthetic 1080p pair (%d x %d regions, %d tentatives), no database attached; %d rounds of fresh processes, alternating"
               % (*runs["this build"][0]["regions"], runs["this build"][0]["tentatives"], ROUNDS))
    for name, rs in runs.items():
        if rs:
            v = [x["match"]["mean"] for x in rs]
            out.append("  %-11s %s ms   spread (max - min) %.4f" % (name, " ".join("%.4f" % x for x in v), max(v) - min(v)))
    out.append("  scopes the DISTRACTOR timer counted in this build's runs: %s" % " ".join(str(x["distractor_scopes"]) for x in runs["this build"]))
    out.append("")
    if "--skip-bench" not in args:
        runs = {"this build": [], "parent": []}
        for _ in range(ROUNDS):
            runs["this build"].append(spawn("bench", reps))
            if other:
                runs["parent"].append(spawn("bench", reps, other))
        key = bench_figure(runs["this build"][0])[0]
        out.append("bench.py --gpus 1 --steps 10 --warmup 2, no database attached, %s; %d rounds of fresh processes, alternating" % (key, ROUNDS))
        for name, rs in runs.items():
            if rs:
                v = [float(x[key]) for x in rs]
                out.append("  %-11s %s   spread (max - min) %.4g" % (name, " ".join("%.5g" % x for x in v), max(v) - min(v)))
        on = spawn("bench_db", reps)
        out.append("  with a 2^20-row random database attached to the pipeline: %.5g" % float(on[key]))
        out.append("")
    g = spawn("graf", reps)
    out += ["graf1 / graf6 (tests/golden, 800 x 640), mods_match_pair_dev: one view, homography, ratio 0.8, RANSAC seed pinned; database: %d descriptors"
            % g["db_rows"], "of the project's own synthetic textures (tests/synth.py, %s), described by the library - no natural-image corpus is at hand;"
            % ", ".join("%d x %d" % s for s in TEXTURES), "true = within err_threshold of the homography the default run without a database verified",
            "%-15s %-9s %-14s %-11s %-6s %-8s %-9s %-8s" % ("FixedRegNumber", "database", "described", "tentatives", "true", "unique", "verified", "samples")]
    for row in g["rows"]:
        out.append("%-15s %-9s %-14s %-11d %-6d %-8d %-9d %-8d" % (row["keep"] or "default", "on" if row["on"] else "off", "%d / %d" % tuple(row["described"]),
                                                              row["tentatives"], row["true"], row["unique"], row["inliers"], row["samples"]))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "distractor_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
