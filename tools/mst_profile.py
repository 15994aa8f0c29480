#!/usr/bin/env python3
"""A cohort of N SARS-CoV-2-sized consensus sequences (29,903 positions), set once, and its minimum spanning forest found REPS times:
the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mst_profile.py device KIND N [REPS]
which gives the times of cohort_pairs_kernel, cohort_row_best_kernel and the two component kernels per call of bk_cohort_mst
(DESIGN.md section Y).  KIND is `related` (the cohort of tools/cohort_profile.py: a base sequence, some twenty substitutions and a
run of N per sample; few rounds) or `ruler` (a chain: sample i is sample i - 1 plus 1 + the trailing zeros of i fresh
substitutions, rows shuffled; about log2 N rounds).  Without the profiler it prints the wall time of each call (host clock around a
call that ends in a synchronise) and checks the forest against the host twin's.
    python tools/mst_profile.py host KIND N [REPS] [THREADS]
times the host twin (cohort_pack_host and cohort_mst_host: Prim) on THREADS threads, 16 by default, on the same letters: the yardstick.
--mst-min-breadth's default decides what is an edge: min_compared = ceil(0.9 x positions)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import hostlib  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "device"
KIND = sys.argv[2] if len(sys.argv) > 2 else "related"
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
THREADS = int(sys.argv[5]) if len(sys.argv) > 5 else 16
POSITIONS = 29903
ACGT = np.frombuffer(b"ACGT", np.uint8)


def related(n, positions, seed=17):
    rng = np.random.default_rng(seed)
    a = np.tile(ACGT[rng.integers(0, 4, positions)], (n, 1))
    for s in range(n):
        at = rng.integers(0, positions, 20)
        a[s, at] = ACGT[rng.integers(0, 4, 20)]
        lo = int(rng.integers(0, positions - 300))
        a[s, lo:lo + int(rng.integers(0, 300))] = ord("N")
    return np.ascontiguousarray(a)


def ruler(n, positions, seed=19):
    rng = np.random.default_rng(seed)
    order = rng.permutation(positions)
    a = np.empty((n, positions), np.uint8)
    a[0] = ACGT[rng.integers(0, 4, positions)]
    used = 0
    for i in range(1, n):
        g = (i & -i).bit_length()
        a[i] = a[i - 1]
        at = order[np.arange(used, used + g) % positions]
        a[i, at] = ACGT[(np.searchsorted(ACGT, a[i, at]) + 1) % 4]
        used += g
    return np.ascontiguousarray(a[rng.permutation(n)])


a = {"related": related, "ruler": ruler}[KIND](N, POSITIONS)
need = hostlib.cohort_min_compared(0.9, POSITIONS)
if MODE == "host":
    best = None
    for rep in range(REPS):
        t0 = time.perf_counter()
        edges, near = hostlib.cohort_mst(a, need, threads=THREADS)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        print("host %s n=%d threads=%d rep %d: %.3f ms" % (KIND, N, THREADS, rep, dt * 1e3))
    print("host %s n=%d threads=%d best %.3f ms, %d edges, longest %d" % (KIND, N, THREADS, best * 1e3, len(edges), int(edges[:, 2].max()) if len(edges) else 0))
else:
    ix = hostlib.HostIndex.load(os.path.join(ROOT, "tests", "golden", "hpv.bkdb"))
    eng = ix.engine()
    eng.cohort_set(a)
    best = None
    for rep in range(REPS):
        t0 = time.perf_counter()
        edges, near, rounds = eng.cohort_mst(need)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        print("device %s n=%d rep %d bk_cohort_mst: %.3f ms, %d rounds" % (KIND, N, rep, dt * 1e3, rounds))
    print("device %s n=%d best call %.3f ms, %d edges, %d rounds, longest %d" % (KIND, N, best * 1e3, len(edges), rounds, int(edges[:, 2].max()) if len(edges) else 0))
    he, hn = hostlib.cohort_mst(a, need, threads=THREADS)
    if not (np.array_equal(edges, he) and np.array_equal(near, hn)):
        raise SystemExit("mst_profile: the device's forest differs from the host twin's")
    print("device %s n=%d: equal to the host twin" % (KIND, N))
    eng.close()
    ix.close()
