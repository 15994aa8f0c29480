"""More records in one push than one trip of the grid: the second and later trips of chimera_scan_kernel's grid-stride loop and the
three paths of its per-wave queue that only a later trip reaches (the carry-over, the drain at 64 waiting records, the walk of what
remains) -- tests/test_gpu_copyback_trips.py's method and tests/test_gpu_grid_trips.py's model of the queue.

One push of ceil(2.5 x CUs x 8 x 256) records of 64 bases on the chimera tests' crafted genome at k = 21: a list of P = 101 distinct
records repeated cyclically, so that no wave meets the same mixture twice.  Every result is additive over the records, so what is
expected is the restatement's result of the P records times each record's multiplicity.  All comparisons are exact."""
import random

import numpy as np
import pytest

from bronko_amd import pack_reads
from bronko_amd.hostlib import HostIndex
from tests import chimera_cases, chimeras_ref, indel_cases
from tests.chimeras_ref import L, R
from tests.test_gpu_grid_trips import _queue_walk, _scaled

pytestmark = pytest.mark.gpu
K, N_LEN = 21, 64
M = 2
P = 101
SIDES = ((L, R), (L, L), (R, R), (R, L))


def _draw(g, rng, kind, sides):
    t = g.text
    lo = [f + 150 for f in g.first]
    hi = [f + len(s) - 150 for f, s in zip(g.first, g.seqs)]
    s, q = rng.sample((0, 1, 2, 4, 5), 2)                          # (craftD is short and holds a run of N)
    x, y = rng.randrange(lo[s], hi[s]), rng.randrange(lo[q], hi[q])
    la = rng.randrange(K, N_LEN - K + 1)
    while "N" in t[x:x + N_LEN + 40]:                              # (the reads of one sequence are cut clear of the runs of N)
        x = rng.randrange(lo[s], hi[s])
    if kind == "junction":
        r = chimera_cases.chimera_read(t, x, sides[0], y, sides[1], la, N_LEN - la, tuple(rng.sample(range(K), rng.choice((0, 0, 1)))))
    elif kind == "mismatched":                                     # a junction with three substitutions between the anchors
        r = chimera_cases.chimera_read(t, x, sides[0], y, sides[1], 32, N_LEN - 32, (K, K + 1, 2 * K))
    elif kind == "deletion":                                       # a record of one sequence that is no spanning one
        r = indel_cases.mut_read(t, x, N_LEN, dele=(x + la, rng.choice((1, 5, 40))))
    elif kind == "plain":
        r = indel_cases.mut_read(t, x, N_LEN, subs=tuple(rng.sample(range(K, 2 * K), rng.choice((0, 1, 2)))))
    else:
        assert kind == "foreign"
        r = indel_cases._rand(rng, N_LEN)
    r = r.replace("N", "A")
    return chimeras_ref.revcomp(r) if rng.random() < 0.5 else r


def _is(g, rec, kind):
    c = chimeras_ref.chimera_events(g, [rec], M).counters
    if kind == "junction":
        return c["supporting"] == 1
    if kind == "mismatched":
        return c["discordant"] == 1
    if kind == "foreign":
        return c["same_strand"] == 0 and c["crossed"] == 0
    if kind == "deletion":
        return c["same_strand"] == 1 and c["ref_spanning"] == 0
    return c["ref_spanning"] == 1


def _records(g):
    """(the P distinct records, which of them the kernel queues, which of them support an event)"""
    rng = random.Random(47)
    slow = ["junction"] * 36 + ["mismatched"] * 4
    rest = ["plain"] * 44 + ["deletion"] * 12 + ["foreign"] * 5
    rng.shuffle(slow)
    rng.shuffle(rest)
    n_slow = len(slow)
    assert n_slow + len(rest) == P
    kinds = [slow.pop() if (j + 1) * n_slow // P > j * n_slow // P else rest.pop() for j in range(P)]   # the queued ones evenly spread
    recs, seen = [], set()
    for j, kd in enumerate(kinds):
        for _ in range(200):
            r = _draw(g, rng, kd, SIDES[j % 4])                    # all four orientations in turn
            if r not in seen and _is(g, r, kd):
                break
        else:
            raise AssertionError("no record of kind %s" % kd)
        seen.add(r)
        recs.append(r)
    return recs, np.array([kd in ("junction", "mismatched") for kd in kinds]), np.array([kd == "junction" for kd in kinds])


def test_two_and_a_half_trips_of_the_grid_in_one_push():
    import torch
    seqs = chimera_cases.crafted_genome(K)
    g = chimeras_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], K)
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

    a, b = chimeras_ref.chimera_events(g, recs, M), chimeras_ref.chimera_events(g, recs[:rem], M)
    both = chimeras_ref.Result({key: [q * f + b.events.get(key, [0, 0])[0], q * r + b.events.get(key, [0, 0])[1]] for key, (f, r) in a.events.items()},
                               _scaled(a.span, b.span, q).tolist(), {name: q * a.counters[name] + b.counters[name] for name in a.counters})
    assert set(b.events) <= set(a.events) and len(a.events) >= 30 and all(v > 0 for v in a.counters.values())
    assert {(key[1], key[3]) for key in a.events} == set(SIDES)
    assert both.counters["supporting"] == int(supporting[np.arange(n) % P].sum()) < int(queued[np.arange(n) % P].sum()) == both.counters["crossed"]

    words, lens = pack_reads([r.encode() for r in recs], K)
    assert words.shape == (P, 4) and (lens == N_LEN).all()
    idx = np.arange(n) % P
    ix = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in seqs])])
    eng = ix.engine()
    try:
        eng.chimeras_enable(M)
        eng.sample_begin()
        eng.push_reads(0, words[idx], lens[idx])
        eng.sample_finalize(1)
        eng.sample_chimeras(1)
        summ, rows = eng.download_chimeras()
        want = chimeras_ref.table_rows(g, both)
        assert rows == want, ([r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
        got = (summ.records, summ.same_strand, summ.ref_spanning, summ.crossed, summ.supporting, summ.discordant)
        assert got == chimeras_ref.counters_tuple(both) and summ.records == n
        assert summ.candidates == summ.reported == len(want) and summ.overflow == 0
        span = eng.download_chimera_span()
        sums = np.array(both.span_sums()[:g.cells], np.int64).astype(np.uint32)
        assert np.array_equal(span, sums), np.flatnonzero(span != sums)[:5]
    finally:
        eng.close()
        ix.close()
