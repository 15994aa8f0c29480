"""The cohorts of the --mst tests.  Rows are shuffled with a fixed seed, so that sample order and relatedness are unrelated.

  related  cohort_ref.cohort as it is: related samples, an all-N sample, identical samples, a pair that differs everywhere; many of
           its forest's edges share a diff with another edge (the tie order), its forests need few rounds
  ruler    a chain: sample i is sample i - 1 plus g(i) fresh substitutions, g the ruler sequence 1, 2, 1, 3, 1, 2, 1, 4, ...: the
           components of a Boruvka round pair up along the chain, so the forest needs about log2 n rounds and merges chains of
           components several labels long.  (With fewer positions than the chain needs, positions are used again: still a valid
           cohort, no longer a ruler.)
  clonal   each sample descends from a random earlier one, with 0 - 3 substitutions and a run of N of its own on top of its
           ancestors': at a high breadth bound it falls apart into many components, with singletons and samples without a nearest
           neighbour
"""
import functools

import numpy as np

from tests import cohort_ref, mst_ref

ACGT = np.frombuffer(b"ACGT", np.uint8)
KINDS = ("related", "ruler", "clonal")


def _rotated(letters, at):
    """The letters with the bases at `at` replaced by the next base (A C G T A); N stays N."""
    code = np.searchsorted(ACGT, letters[at])
    ok = np.isin(letters[at], ACGT)
    letters[at] = np.where(ok, ACGT[(code % 4 + 1) % 4], letters[at])


def ruler(n, positions, seed):
    rng = np.random.default_rng(seed)
    order = rng.permutation(positions)
    a = np.empty((n, positions), np.uint8)
    a[0] = ACGT[rng.integers(0, 4, positions)]
    used = 0
    for i in range(1, n):
        g = 1 + ((i & -i).bit_length() - 1)                      # the ruler sequence: 1 + the trailing zeros of i
        a[i] = a[i - 1]
        _rotated(a[i], order[np.arange(used, used + g) % positions])
        used += g
    return np.ascontiguousarray(a[rng.permutation(n)])


def clonal(n, positions, seed):
    rng = np.random.default_rng(seed)
    a = np.empty((n, positions), np.uint8)
    a[0] = ACGT[rng.integers(0, 4, positions)]
    for i in range(1, n):
        a[i] = a[int(rng.integers(0, i))]
        _rotated(a[i], rng.integers(0, positions, int(rng.integers(0, 4))))
        run = int(rng.integers(0, max(2, positions // 20)))
        start = int(rng.integers(0, positions))
        a[i, start:start + run] = ord("N")
    return np.ascontiguousarray(a[rng.permutation(n)])


@functools.lru_cache(maxsize=None)
def case(kind, n, positions):
    """(letters, diff, compared) of a cohort, computed once and read-only."""
    seed = 7000 * KINDS.index(kind) + 1000 * n + positions
    a = {"related": cohort_ref.cohort, "ruler": ruler, "clonal": clonal}[kind](n, positions, seed)
    d, c = cohort_ref.distances(a)
    for x in (a, d, c):
        x.setflags(write=False)
    return a, d, c


@functools.lru_cache(maxsize=None)
def expected(kind, n, positions, need):
    """(edges, nearest, rounds) of a case by the restatement: Kruskal's edges, checked against the plain Boruvka's."""
    _, d, c = case(kind, n, positions)
    edges = mst_ref.kruskal(d, c, need)
    again, rounds = mst_ref.boruvka(d, c, need)
    assert again == edges                                        # (the forest is unique: two algorithms, one set of edges)
    return edges, mst_ref.nearest(d, c, need), rounds


def needs(positions):
    """The min_compared values of the tests: 0, ceil(0.5 x positions), ceil(0.9 x positions)."""
    return (0, mst_ref.min_compared(0.5, positions), mst_ref.min_compared(0.9, positions))
