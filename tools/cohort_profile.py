#!/usr/bin/env python3
"""A cohort of N related SARS-CoV-2-sized consensus sequences (29,903 positions: a base sequence, some twenty substitutions and a few
hundred N per sample), set once and compared REPS times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cohort_profile.py device N [REPS]
which gives the times of cohort_pack_kernel and cohort_pairs_kernel.  Without the profiler it prints the wall
time of bk_cohort_set and of each bk_cohort_distances (host clock around calls that end in a synchronise; the downloads included).
    python tools/cohort_profile.py host N [REPS] [THREADS]
times the host twin (cohort_distances_host: packing and pairs) on THREADS threads, 16 by default, on the same letters: the yardstick.
`device` also checks its matrices against the host twin's.  With BK_COHORT_SLICE_WORDS set it binds the testing library, which reads
it: 468 makes every tile one slice."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import _ffi, hostlib  # noqa: E402

if os.environ.get("BK_COHORT_SLICE_WORDS"):          # the testing library reads it: 468 words = one slice, what the launch is without slices
    _ffi.use_testing_library(True)

MODE = sys.argv[1] if len(sys.argv) > 1 else "device"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
THREADS = int(sys.argv[4]) if len(sys.argv) > 4 else 16
POSITIONS = 29903


def letters(n, positions, seed=17):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = np.tile(acgt[rng.integers(0, 4, positions)], (n, 1))
    for s in range(n):
        at = rng.integers(0, positions, 20)
        a[s, at] = acgt[rng.integers(0, 4, 20)]
        lo = int(rng.integers(0, positions - 300))
        a[s, lo:lo + int(rng.integers(0, 300))] = ord("N")
    return np.ascontiguousarray(a)


a = letters(N, POSITIONS)
pair_positions = float(N) * N * POSITIONS
if MODE == "host":
    best = None
    for rep in range(REPS):
        t0 = time.perf_counter()
        d, c = hostlib.cohort_distances(a, threads=THREADS)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        print("host n=%d threads=%d rep %d: %.3f ms" % (N, THREADS, rep, dt * 1e3))
    print("host n=%d threads=%d best %.3f ms, %.3e pair-positions/s, largest distance %d" % (N, THREADS, best * 1e3, pair_positions / best, int(d.max())))
else:
    ix = hostlib.HostIndex.load(os.path.join(ROOT, "tests", "golden", "hpv.bkdb"))
    eng = ix.engine()
    t0 = time.perf_counter()
    eng.cohort_set(a)
    print("device n=%d bk_cohort_set: %.3f ms" % (N, (time.perf_counter() - t0) * 1e3))
    best = None
    for rep in range(REPS):
        t0 = time.perf_counter()
        d, c = eng.cohort_distances()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        print("device n=%d rep %d bk_cohort_distances: %.3f ms" % (N, rep, dt * 1e3))
    print("device n=%d best call %.3f ms, %.3e pair-positions/s by the call's wall time, largest distance %d" % (N, best * 1e3, pair_positions / best, int(d.max())))
    hd, hc = hostlib.cohort_distances(a, threads=THREADS)
    if not (np.array_equal(d, hd) and np.array_equal(c, hc)):
        raise SystemExit("cohort_profile: the device's matrices differ from the host twin's")
    print("device n=%d: equal to the host twin" % N)
    eng.close()
    ix.close()
