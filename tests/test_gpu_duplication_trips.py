"""More records in one push than one trip of the grid: the second and later trips of duplication_scan_kernel's grid-stride loop and
the three paths of its per-wave queue that only a later trip reaches (the carry-over, the drain at 64 waiting records, the walk of
what remains) -- tests/test_gpu_junction_trips.py's method and tests/test_gpu_grid_trips.py's model
of the queue.

One push of ceil(2.5 x CUs x 8 x 256) records of 64 bases on HPV16 at k = 21: a list of P = 101 distinct records repeated
cyclically, so that no wave meets the same mixture twice.  Every result is additive over the records, so what is expected is the
restatement's result of the P records times each record's multiplicity.  All comparisons are exact."""
import os
import random

import numpy as np
import pytest

from bronko_amd import pack_reads
from bronko_amd.hostlib import HostIndex
from tests import duplication_cases, duplications_ref, indel_cases
from tests.test_gpu_grid_trips import _queue_walk, _scaled

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, N_LEN = 21, 64
L, M = 33, 2
P = 101


def _draw(g, rng, kind):
    t = g.text
    start = rng.randrange(3200, 7000)
    left = rng.randrange(K, 2 * K + 2)
    bp = start + left
    if kind == "duplication":
        e = rng.choice((33, 34, 64, 200, 1000, 3000))
        r = duplication_cases.dup_read(t, bp, e, left, N_LEN, subs=tuple(rng.sample(range(K), rng.choice((0, 0, 1)))))
    elif kind == "origin":
        r = duplication_cases.origin_read(t, left, N_LEN - left)
    elif kind == "mismatched":                                     # a duplication with three substitutions between the anchors
        r = duplication_cases.dup_read(t, bp, 500, left, N_LEN, subs=(K, K + 1, 2 * K))
    elif kind == "short":
        r = duplication_cases.dup_read(t, bp, rng.choice((1, 5, 32)), left, N_LEN)
    elif kind == "forward":
        r = indel_cases.mut_read(t, start, N_LEN, dele=(bp, rng.choice((1, 40, 300))))
    elif kind == "plain":
        r = indel_cases.mut_read(t, start, N_LEN, subs=tuple(rng.sample(range(K, 2 * K), rng.choice((0, 1, 2)))))
    else:
        assert kind == "foreign"
        r = indel_cases._rand(rng, N_LEN)
    return duplications_ref.revcomp(r) if rng.random() < 0.5 else r


def _is(g, rec, kind):
    res = duplications_ref.duplication_events(g, [rec], L, M)
    c = res.counters
    if kind == "duplication":
        return c["supporting"] == 1
    if kind == "origin":
        return list(res.events) == [(g.cells, g.cells)]
    if kind == "mismatched":
        return c["discordant"] == 1 and duplications_ref.duplication_events(g, [rec], L, 8).counters["supporting"] == 1   # (it reaches the walk)
    if kind == "foreign":
        return c["anchored"] == 0
    return c[{"short": "short", "forward": "forward", "plain": "ref_spanning"}[kind]] == 1


def _records(g):
    """(the P distinct records, which of them the kernel queues, which of them support an event)"""
    rng = random.Random(41)
    slow = ["duplication"] * 32 + ["origin"] * 4 + ["mismatched"] * 4
    rest = ["plain"] * 40 + ["short"] * 8 + ["forward"] * 8 + ["foreign"] * 5
    rng.shuffle(slow)
    rng.shuffle(rest)
    n_slow = len(slow)
    assert n_slow + len(rest) == P
    kinds = [slow.pop() if (j + 1) * n_slow // P > j * n_slow // P else rest.pop() for j in range(P)]   # the queued ones evenly spread
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
    return recs, np.array([kd in ("duplication", "origin", "mismatched") for kd in kinds]), np.array([kd in ("duplication", "origin") for kd in kinds])


def test_two_and_a_half_trips_of_the_grid_in_one_push():
    import torch
    g = duplications_ref.read_fasta(os.path.join(GOLDEN, "HPV16.fa"), K)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * 8
    n = -(-5 * grid * 256 // 2)                                    # ceil(2.5 x CUs x 8 x 256)
    recs, queued, supporting = _records(g)
    assert len(set(recs)) == P and all(len(r) == N_LEN for r in recs)
    q, rem = divmod(n, P)

    # the queue's paths, counted on the host before anything is pushed
    per_trip, drained, carried, left = _queue_walk(queued, n, grid)
    trips, waves = per_trip.shape
    assert trips == 3 and waves == grid * 4
    full = np.arange(trips)[:, None] * waves * 64 + np.arange(waves)[None, :] * 64 + 64 <= n
    assert per_trip[full].min() >= 20 and per_trip[full].max() <= 45
    three = full[2]                                                # the waves that go round three times
    assert three.sum() >= waves // 4 and not drained[0].any()
    assert (drained[1, three] | drained[2, three]).all()           # ... cross 64 on their second or third trip
    assert (carried[1] > 0).all() and (carried[2, three] > 0).all()   # every later trip begins with records waiting
    assert (left > 0).all()                                        # every wave walks a remainder at the end

    a, b = duplications_ref.duplication_events(g, recs, L, M), duplications_ref.duplication_events(g, recs[:rem], L, M)
    both = duplications_ref.Result({key: [q * f + b.events.get(key, [0, 0])[0], q * r + b.events.get(key, [0, 0])[1]] for key, (f, r) in a.events.items()},
                                _scaled(a.span, b.span, q).tolist(), {name: q * a.counters[name] + b.counters[name] for name in a.counters})
    assert set(b.events) <= set(a.events) and len(a.events) >= 30 and all(v > 0 for v in a.counters.values())
    assert both.counters["supporting"] == int(supporting[np.arange(n) % P].sum()) < int(queued[np.arange(n) % P].sum())

    words, lens = pack_reads([r.encode() for r in recs], K)
    assert words.shape == (P, 4) and (lens == N_LEN).all()
    idx = np.arange(n) % P
    ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
    eng = ix.engine()
    try:
        eng.duplications_enable(L, M)
        eng.sample_begin()
        eng.push_reads(0, words[idx], lens[idx])
        eng.sample_finalize(1)
        eng.sample_duplications(1)
        summ, rows = eng.download_duplications()
        want = duplications_ref.table_rows(g, both)
        assert rows == want, ([r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
        got = (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.short_, summ.forward, summ.discordant)
        assert got == duplications_ref.counters_tuple(both) and summ.records == n
        assert summ.candidates == summ.reported == len(want) and summ.overflow == 0
        span = eng.download_duplication_span()
        sums = np.array(both.span_sums()[:g.cells], np.int64).astype(np.uint32)
        assert np.array_equal(span, sums), np.flatnonzero(span != sums)[:5]
    finally:
        eng.close()
        ix.close()
