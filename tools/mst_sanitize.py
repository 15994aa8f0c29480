#!/usr/bin/env python3
"""Build tools/mst_sanitize.cpp with AddressSanitizer and UBSan and run it, on the CPU, over the cohorts of tests/mst_cases.py at
the shapes of tests/test_mst_cpu.py: the host twin of bk_cohort_mst, the rooting and the writer of --mst, and their file against
the restatement's.  Nothing of it is loaded into Python: the program is a child process with its own main."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mst_cases, mst_ref  # noqa: E402

subprocess.run(["make", "-C", os.path.join(ROOT, "bronko_amd", "host"), "sanitize-mst"], check=True)
prog = os.path.join(ROOT, "bronko_amd", "bin", "mst_sanitize")
env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
runs = 0
with tempfile.TemporaryDirectory() as d:
    raw, out = os.path.join(d, "letters.bin"), os.path.join(d, "out.mst.tsv")
    for kind in mst_cases.KINDS:
        for n in (1, 2, 3, 63, 64, 65, 130):
            for positions in (129, 700, 4999):
                a = mst_cases.case(kind, n, positions)[0]
                a.tofile(raw)
                for need in mst_cases.needs(positions):
                    res = subprocess.run([prog, raw, str(n), str(positions), str(need), out], env=env, stdout=subprocess.DEVNULL)
                    if res.returncode != 0:
                        sys.exit("mst_sanitize failed at %s n = %d positions = %d min_compared = %d (exit status %d)" % (kind, n, positions, need, res.returncode))
                    edges, near, _ = mst_cases.expected(kind, n, positions, need)
                    if open(out, "rb").read() != mst_ref.mst_text(["s%d" % i for i in range(n)], edges, near, 0.5, need):
                        sys.exit("mst_sanitize: the file differs from the restatement's at %s n = %d positions = %d min_compared = %d" % (kind, n, positions, need))
                    runs += 1
print("mst_sanitize: clean, %d runs" % runs)
