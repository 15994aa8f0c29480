#!/usr/bin/env python3
"""Build tools/breakends_sanitize.cpp with AddressSanitizer and UBSan and run it over the crafted records of tests/breakend_cases.py
(k = 21 and 31), on the CPU; after the breakend twin the program runs the twins of the other five event passes over the same records.
Nothing of it is loaded into Python: the program is a child process with its own main."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import breakend_cases  # noqa: E402

subprocess.run(["make", "-C", os.path.join(ROOT, "bronko_amd", "host"), "sanitize-breakends"], check=True)
prog = os.path.join(ROOT, "bronko_amd", "bin", "breakends_sanitize")
with tempfile.TemporaryDirectory() as d:
    for k in (21, 31):
        fa, rd = (os.path.join(d, n) for n in ("g.fa", "reads.txt"))
        with open(fa, "w") as f:
            for name, s in breakend_cases.crafted_genome():
                f.write(">%s\n%s\n" % (name, s))
        with open(rd, "w") as f:
            f.write("".join(r + "\n" for _, r, _ in breakend_cases.crafted_cases(k)[0]))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        res = subprocess.run([prog, str(k), fa, rd, os.path.join(d, "out.tsv")], env=env)
        if res.returncode != 0:
            sys.exit("breakends_sanitize failed at k = %d (exit status %d)" % (k, res.returncode))
print("breakends_sanitize: clean")
