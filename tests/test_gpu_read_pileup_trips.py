"""More rows in the store than one trip of read_pileup_count_kernel's grid: the second and later trips of its grid-stride loop.

One push of ceil(2.5 x CUs x 8 x 256) records of 64 bases on HPV16 at k = 21, built as tests/test_gpu_grid_trips.py builds its push:
a list of P distinct records (P prime) repeated cyclically, so that no wave meets the same mixture twice.  Every record is placed --
plain or with one to eight substitutions, along or against the reference --, so the store holds as many rows as records.  The result
is additive over the rows: what is expected is the restatement's result of the P records times each record's multiplicity; the full
list never goes through the restatement.  All comparisons are exact."""
import os
import random

import numpy as np
import pytest

from bronko_amd import hostlib, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import indels_ref, linkage_ref, read_pileup_ref
from tests.test_gpu_grid_trips import K, M, N_LEN, _draw, _is

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _records(g):
    """P = 97 distinct placed records"""
    rng = random.Random(33)
    kinds = ["plain"] * 17 + ["subs%d" % n for n in range(1, 9) for _ in range(10)]
    rng.shuffle(kinds)
    recs, seen = [], set()
    for kd in kinds:
        for _ in range(200):
            r = _draw(g, rng, kd)
            if r not in seen and _is(g, r, kd):
                break
        else:
            raise AssertionError("no record of kind %s" % kd)
        seen.add(r)
        recs.append(r)
    return recs


def test_two_and_a_half_trips_of_the_count_kernels_grid():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * 8                                                 # row_grid(rows, 256, CUs, 8)
    n = -(-5 * grid * 256 // 2)
    g = indels_ref.read_fasta(os.path.join(GOLDEN, "HPV16.fa"), K)
    recs = _records(g)
    P = len(recs)
    assert P == 97 and len(set(recs)) == P and all(len(r) == N_LEN for r in recs)
    rows = [linkage_ref.place(g, r, M)[1] for r in recs]
    assert all(r is not None for r in rows) and {r[2] for r in rows} == {0, 1} and max(len(r[3]) for r in rows) == 8
    q, rem = divmod(n, P)
    assert n > 2 * grid * 256 and q > 1000
    words, lens = pack_reads([r.encode() for r in recs], K)
    idx = np.arange(n) % P
    ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
    eng = ix.engine()
    try:
        eng.linkage_enable(M)
        eng.sample_begin()
        eng.push_reads(0, words[idx], lens[idx])
        eng.sample_finalize(1)
        for E in (10, N_LEN // 2, 0):                              # two stretches near the ends; every cell (n = 2 E); none
            want = (q * read_pileup_ref.read_pileup(g, rows, E).astype(np.int64) + read_pileup_ref.read_pileup(g, rows[:rem], E)).astype(np.uint32)
            eng.sample_read_pileup(E)
            summ, cells = eng.download_read_pileup()
            assert np.array_equal(cells, want), (E, np.argwhere(cells != want)[:5].tolist())
            assert (summ.rows, summ.n_cells, summ.end_dist, summ.bases) == (n, g.cells, E, n * N_LEN)
            assert summ.covered == int((want[:, :8].sum(axis=1) > 0).sum()) and want[:, :8].sum(axis=1).max() > n // 4
        print("%d CUs, %d rows in the store" % (cus, n))
        twin = hostlib.read_pileup_count(ix, 0, eng.download_link_rows(raw=True), 0)
        assert np.array_equal(twin, want)
    finally:
        eng.close()
        ix.close()
