"""ms per mods_orsa_f call for the recorded fixture sizes (tests/golden/orsa_ref.npz inputs), split into host 7-point solves,
scoring round trips, scoring kernels (HIP events) and replay, with the kernel's models per second; the host scoring path of the
same call beside it.  Warm-up call first, then REPEATS timed calls: median and min-max."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_cpu_orsa as cpu  # noqa: E402

pkg = cpu.pkg
REPEATS = int(os.environ.get("REPEATS", "5"))


def timed(u6, meta, on_device, **kw):
    pkg.orsa_f(u6, None, int(meta[1]), int(meta[2]), seed_time=int(meta[3]), on_device=on_device, **kw)   # warm-up
    rows = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = pkg.orsa_f(u6, None, int(meta[1]), int(meta[2]), seed_time=int(meta[3]), on_device=on_device, **kw)
        wall = 1e3 * (time.perf_counter() - t)
        p = pkg.orsa_last_profile()
        rows.append((wall, p["solve"], p["score"], p["kernel"], p["replay"], p["launches"], r["stats"]))
    return rows


def summary(rows, i):
    v = np.array([r[i] for r in rows])
    return "%.1f [%.1f-%.1f]" % (np.median(v), v.min(), v.max())


cases = sys.argv[1:] or cpu.CASES
print("case n | iters models rewinds | device call ms | solve | score round trips | kernels | replay | launches | "
      "kernel Mmodel/s | host-path call ms")
for name in cases:
    u6, meta = cpu.case_inputs(name)
    d = timed(u6, meta, True)
    h = timed(u6, meta, False)
    st = d[0][6]
    kern = np.median([r[3] for r in d])
    print("%s %d | %d %d %d | %s | %s | %s | %s | %s | %d | %.3f | %s" % (
        name, len(u6), st[0], st[1], st[2], summary(d, 0), summary(d, 1), summary(d, 2), summary(d, 3), summary(d, 4), d[0][5],
        st[1] / kern / 1e3 if kern > 0 else 0, summary(h, 0)), flush=True)
