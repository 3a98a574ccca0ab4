"""Exhaustive check of the device's (float)log10((double)x) - ocml's double log10 rounded to float, what orsa_score_kernel
evaluates for each sorted error - against glibc's, which the reference's NFA scan uses (orsa.cpp:560): every non-negative float
bit pattern 0x00000000 .. 0x7fffffff (zero, subnormals, normals, inf, the NaNs).  Prints the mismatch count and any bit
patterns; the run's output is kept in profiles/orsa_log10_sweep.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
t = time.time()
total, lists = 0, []
step = 1 << 28
for b in range(0, 1 << 31, step):
    bad, lst = pkg.orsa_log10_sweep(b, step)
    total += bad
    lists.extend(int(v) for v in lst)
    print("[0x%08x, 0x%08x): %d mismatches" % (b, b + step, bad), flush=True)
print("all 2^31 non-negative float bit patterns: %d mismatches (%.1f s)" % (total, time.time() - t))
for v in lists[:64]:
    print("  mismatch at 0x%08x" % v)
sys.exit(0 if total == 0 else 1)
