"""CLAHE cost on the MI355X (profiles/clahe_timing.txt).

  kernels        run under `rocprofv3 --kernel-trace --stats`: mods_clahe_dev (u8 -> fp32) on 32 x 1920 x 1080 and on 2 x 4096 x 4096,
                 REPEATS calls each, and a plain pair pipeline with ONE GPU worker (16 pairs per batch: its u8_to_f32_kernel launches
                 convert the same 32-image batches without other workers' kernels beside them)
  rates          pipeline pairs/s at the bench shape (4 GPU workers x 16 pairs, 8 verify workers, pinned 8-bit 1080p pairs): plain,
                 with CLAHE, and plain on images equalised beforehand (tests/clahe_ref.py: the same regions as the CLAHE run, so the
                 difference to it is what CLAHE itself costs), alternated, with the mean region counts; JSON to stdout
  report T R     kernel statistics from the trace directory T (kernel_trace CSV) + the rates JSON file R -> stdout"""
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = int(os.environ.get("REPEATS", "20"))
KERNELS = ("clahe_lut_kernel", "clahe_apply_kernel", "u8_to_f32_kernel")


def _pkg():
    import __graft_entry__ as ge
    return ge.load_package()


def _pairs(w, h, n=6):
    import synth
    return [np.stack([a, b]).astype(np.uint8) for a, b, _ in (synth.pair(w, h, seed=2000 + i) for i in range(n))]


def _pipeline(pkg, stacks, clahe, n_sub, warm=64, gpu_workers=4):
    w, h = stacks[0].shape[2], stacks[0].shape[1]
    pinned = []
    for x in stacks:
        b = pkg.PinnedBuffer(x.shape, np.uint8)
        b.array[...] = x
        pinned.append(b)
    pkg.ransac_pin_seed(12345)
    pipe = pkg.Pipeline(0, w, h, pkg.PairParams.default(), gpu_workers, 8, 16, clahe=clahe)

    def run(n):
        out, pending = [], 0
        for i in range(n):
            if pending >= pipe.capacity - 1:
                out.append(pipe.next()[0]); pending -= 1
            pipe.submit_host(pinned[i % len(pinned)].ptr.value, i, u8=True); pending += 1
        while pending:
            out.append(pipe.next()[0]); pending -= 1
        return out
    run(warm)
    t = time.perf_counter()
    res = run(n_sub)
    dt = time.perf_counter() - t
    pipe.close()
    for b in pinned:
        b.close()
    return n_sub / dt, float(np.mean([r.n_described[0] + r.n_described[1] for r in res]))


def kernels():
    import torch
    pkg = _pkg()
    for w, h, n in ((1920, 1080, 32), (4096, 4096, 2)):
        ctx = pkg.Context(0, w, h, 1)
        src = torch.from_numpy(np.stack([_pairs(w, h, 1)[0][k % 2] for k in range(n)])).cuda()
        dst = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(REPEATS + 1):
            ctx.clahe_dev(src.data_ptr(), n, w, h, dst.data_ptr(), f32=True)
        ctx.close()
        del src, dst
    _pipeline(pkg, _pairs(1920, 1080), None, 128, gpu_workers=1)


def rates():
    pkg = _pkg()
    import clahe_ref
    stacks = _pairs(1920, 1080)
    equalised = [np.stack([clahe_ref.clahe(x) for x in s]) for s in stacks]
    out = {"plain": [], "clahe": [], "equalised": []}
    regions = {}
    for _ in range(2):
        for mode in ("plain", "clahe", "equalised"):
            r, reg = _pipeline(pkg, equalised if mode == "equalised" else stacks,
                               pkg.ClaheParams.reference() if mode == "clahe" else None, 512)
            out[mode].append(round(r, 1))
            regions[mode] = round(reg, 1)
    print(json.dumps({"pairs_per_s": out, "mean_regions_per_pair": regions}))


def report(trace_dir, rates_file):
    rows = {}
    for fn in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            for r in csv.DictReader(f):
                name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
                if name is None:
                    continue
                key = (name, int(r.get("Grid_Size_X", 0)), int(r.get("Grid_Size_Y", 0)))
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    shape = {(64 * 1024, 32): "32 x 1080p", (68 * 256, 32): "32 x 1080p", (64 * 1024, 2): "2 x 4096^2", (256 * 256, 2): "2 x 4096^2",
             (1024 * 256, 1): "one 1080p pair (2 images)"}
    print("kernel | launch shape | grid | launches | median us | min us")
    med = {}
    for (name, gx, gy), v in sorted(rows.items()):
        m = statistics.median(v)
        med[(name, gx, gy)] = m
        print("%s | %s | %d x %d | %d | %.1f | %.1f" % (name, shape.get((gx, gy), "?"), gx, gy, len(v), m, min(v)))
    lut = med.get(("clahe_lut_kernel", 64 * 1024, 32))
    app = med.get(("clahe_apply_kernel", 68 * 256, 32))
    cvt = med.get(("u8_to_f32_kernel", 1024 * 256, 1))
    if lut and app and cvt:
        mb_u8, mb_f32 = 32 * 1920 * 1080 / 1e6, 32 * 1920 * 1080 * 4 / 1e6
        print("32 x 1080p batch: CLAHE lut %.1f + apply %.1f = %.1f us against u8_to_f32 16 x %.1f = %.1f us: ratio %.2f" %
              (lut, app, lut + app, cvt, 16 * cvt, (lut + app) / (16 * cvt)))
        print("  apply moves %.0f MB read + %.0f MB written: %.2f TB/s; lut reads %.0f MB: %.2f TB/s" %
              (mb_u8, mb_f32, (mb_u8 + mb_f32) / app, mb_u8, mb_u8 / lut))
    if rates_file and os.path.exists(rates_file):
        r = json.load(open(rates_file))
        print("pipeline, bench shape (4 GPU workers x 16 pairs, 8 verify workers, pinned 8-bit 1920 x 1080 pairs), 512 pairs per run,"
              " runs alternated: plain %s, CLAHE %s, plain on pre-equalised images %s pairs/s; mean regions per pair plain %s, CLAHE %s,"
              " pre-equalised %s" % (r["pairs_per_s"]["plain"], r["pairs_per_s"]["clahe"], r["pairs_per_s"]["equalised"],
                                     r["mean_regions_per_pair"]["plain"], r["mean_regions_per_pair"]["clahe"],
                                     r["mean_regions_per_pair"]["equalised"]))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "kernels":
        kernels()
    elif cmd == "rates":
        rates()
    elif cmd == "report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        print(__doc__)
        sys.exit(2)
