"""ms per mods_orsa_h call on synthetic planar scenes (tests/orsa_h_ref.py: 640 x 480, sigma 1 px, uniform outliers) of 200, 1000
and 3000 tentatives at 30 % and 60 % inliers: the whole call, the mapping of the samples, the scoring round trips, the scoring
kernels (HIP events: solve phase, keys, sort, NFA scan) and the replay; beside it mods_loransac_h on the same list and the host
path of the same call.  Warm-up call first, then REPEATS timed calls: median and min-max.  Writes profiles/orsa_h_timing.txt
(or the file named by OUT)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orsa_h_ref as ref  # noqa: E402
import test_cpu_orsa_h as cpu  # noqa: E402

pkg = cpu.pkg
REPEATS = int(os.environ.get("REPEATS", "5"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "orsa_h_timing.txt"))
SEED = 4242


def timed_orsa(u6, on_device):
    pkg.orsa_h(u6, None, ref.W, ref.H, seed_time=SEED, on_device=on_device)   # warm-up
    rows = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = pkg.orsa_h(u6, None, ref.W, ref.H, seed_time=SEED, on_device=on_device)
        wall = 1e3 * (time.perf_counter() - t)
        p = pkg.orsa_last_profile()
        rows.append((wall, p["solve"], p["score"], p["kernel"], p["replay"], p["launches"], r))
    return rows


def timed_loransac(u6):
    pkg.loransac_h(u6, None, seed_time=SEED)   # warm-up
    rows = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = pkg.loransac_h(u6, None, seed_time=SEED)
        rows.append((1e3 * (time.perf_counter() - t), r))
    return rows


def summary(rows, i):
    v = np.array([r[i] for r in rows])
    return "%.1f [%.1f-%.1f]" % (np.median(v), v.min(), v.max())


lines = ["# tools/orsa_h_timing.py: ms per call, median [min-max] of %d after a warm-up; synthetic planar scenes 640 x 480, sigma 1 px" % REPEATS,
         "# columns: n, inliers in % | iterations models rewinds | mods_orsa_h call | sample mapping | scoring round trips | scoring kernels "
         "(HIP events) | replay | launches | kernel models/s (millions) | log10 nfa, subset, thr_px | mods_loransac_h call, inliers | "
         "mods_orsa_h on the host path"]
for n in (200, 1000, 3000):
    for ratio in (0.3, 0.6):
        u6, inl, _ = ref.scene(n, ratio, 1.0, 1000 + n + int(100 * ratio))
        d = timed_orsa(u6, True)
        lo = timed_loransac(u6)
        h = timed_orsa(u6, False)
        r = d[0][6]
        kern = np.median([x[3] for x in d])
        lines.append("%d %d | %d %d %d | %s | %s | %s | %s | %s | %d | %.3f | %.1f, %d, %.2f | %s, %d | %s" % (
            n, round(100 * ratio), r["stats"][0], r["stats"][1], r["stats"][2], summary(d, 0), summary(d, 1), summary(d, 2), summary(d, 3),
            summary(d, 4), d[0][5], r["stats"][1] / kern / 1e3 if kern > 0 else 0, r["log_nfa"], len(r["index"]), r["thr_px"],
            summary(lo, 0), lo[0][1][2], summary(h, 0)))
        print(lines[-1], flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
