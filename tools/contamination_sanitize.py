#!/usr/bin/env python3
"""Build tools/contamination_sanitize.cpp with AddressSanitizer and UBSan and run it, on the CPU, over the cohorts of
tests/contamination_ref.py at the shapes of tests/test_contamination_cpu.py: the host twins of the mask kernel and of the explained
kernel, the scanner and the three writers of --contamination, and their files against the restatement's.  Nothing of it is loaded
into Python: the program is a child process with its own main."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cohort_ref, contamination_ref  # noqa: E402

subprocess.run(["make", "-C", os.path.join(ROOT, "bronko_amd", "host"), "sanitize-contamination"], check=True)
prog = os.path.join(ROOT, "bronko_amd", "bin", "contamination_sanitize")
env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
runs = 0
with tempfile.TemporaryDirectory() as d:
    raw, rawm, out = os.path.join(d, "letters.bin"), os.path.join(d, "masks.bin"), os.path.join(d, "out")
    for n in (1, 2, 3, 63, 64, 65, 130):
        for positions in (1, 63, 64, 65, 129, 4999):
            a, m = contamination_ref.cohort(n, positions, 1000 * n + positions)
            a.tofile(raw)
            m.tofile(rawm)
            diff, compared = cohort_ref.distances(a)
            ex, sites = contamination_ref.explained(a, m)
            names = ["s%d" % i for i in range(n)]
            for block, s, p in ((1, 1, 0.0), (2, 3, 0.75), (50, 1, 1.0)):
                res = subprocess.run([prog, raw, rawm, str(n), str(positions), str(block), str(s), repr(p), out], env=env, stdout=subprocess.DEVNULL)
                where = "n = %d positions = %d block = %d S = %d P = %g" % (n, positions, block, s, p)
                if res.returncode != 0:
                    sys.exit("contamination_sanitize failed at %s (exit status %d)" % (where, res.returncode))
                want = {".explained.tsv": contamination_ref.explained_text(names, ex),
                        ".contamination.tsv": contamination_ref.contamination_text(names, diff, compared, ex, sites, 10, 0.03, s, p),
                        ".mixture.tsv": contamination_ref.mixture_text(names, diff, ex, sites, 10, 0.03, s, p)}
                for suffix, text in want.items():
                    if open(out + suffix, "rb").read() != text:
                        sys.exit("contamination_sanitize: %s differs from the restatement's at %s" % (suffix, where))
                runs += 1
print("contamination_sanitize: clean, %d runs" % runs)
