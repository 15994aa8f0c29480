"""More records in one push than one trip of the grid: the second and later trips of breakend_scan_kernel's grid-stride loop and the
three paths of its per-wave queue that only a later trip reaches (the carry-over, the drain at 64 waiting records, the walk of what
remains) -- tests/test_gpu_chimera_trips.py's method and tests/test_gpu_grid_trips.py's model of the queue.

One push of ceil(2.5 x CUs x 8 x 256) records of 64 bases on the breakend tests' crafted genome at k = 21: a list of P = 101 distinct
records repeated cyclically, so that no wave meets the same mixture twice.  Once with about 40 % of the records anchored at one end
only, once with all of them.  Every result is additive over the records, so what is expected is the restatement's result of the P
records times each record's multiplicity.  All comparisons are exact."""
import random

import numpy as np
import pytest

from bronko_amd import pack_reads
from bronko_amd.hostlib import HostIndex
from tests import breakend_cases, breakends_ref
from tests.breakends_ref import L, R
from tests.test_gpu_grid_trips import _queue_walk, _scaled

pytestmark = pytest.mark.gpu
K, N_LEN = 21, 64
C, M = 20, 2
P = 101
TALLY_OF = {"breakend": "supporting", "short": "short", "mismatched": "discordant", "hanging": "unplaced"}


def _draw(g, rng, kind, side):
    t = g.text
    s = rng.randrange(len(g.seqs))
    lo, hi = g.first[s] + 100, g.first[s] + len(g.seqs[s]) - 100
    x = rng.randrange(lo, hi)
    while "N" in t[x - 80:x + 80]:                                 # (clear of the run of N)
        x = rng.randrange(lo, hi)
    at = (lambda o: o) if side == L else (lambda o: N_LEN - 1 - o)
    if kind == "breakend":
        r = breakend_cases.clipped(t, rng, x, side, N_LEN, rng.randrange(25, N_LEN - K + 1))
    elif kind == "short":                                          # (the substitution breaks the far end's third and fourth k-mer)
        r = breakend_cases.sub(breakend_cases.clipped(t, rng, x, side, N_LEN, rng.randrange(17, 20)), at(N_LEN - 30))
    elif kind == "mismatched":                                     # the anchor is the second try, three substitutions in front of it
        r = breakend_cases.sub(breakend_cases.clipped(t, rng, x, side, N_LEN, 25), at(3), at(5), at(7))
    elif kind == "hanging":                                        # eight bases hang over the sequence's border
        f, e = g.first[s], g.first[s] + len(g.seqs[s])
        r = (breakend_cases.foreign(rng, 8) + t[f:f + 31] + breakend_cases.foreign(rng, 25, avoid_head=t[f + 31:f + 39]) if side == L else
             breakend_cases.foreign(rng, 25, avoid_tail=t[e - 39:e - 31]) + t[e - 31:e] + breakend_cases.foreign(rng, 8))
    elif kind == "deletion":
        cut = rng.choice((1, 5, 40))
        r = t[x:x + 32] + t[x + 32 + cut:x + 64 + cut]
    elif kind == "plain":
        r = breakend_cases.sub(t[x:x + N_LEN], *rng.sample(range(K, 2 * K), rng.choice((0, 1, 2))))
    else:
        assert kind == "foreign"
        r = breakend_cases._rand(rng, N_LEN)
    return breakends_ref.revcomp(r) if rng.random() < 0.5 else r


def _is(g, rec, kind):
    c = breakends_ref.breakend_events(g, [rec], C, M).counters
    if kind in TALLY_OF:
        return c[TALLY_OF[kind]] == 1
    if kind == "plain":
        return c["ref_spanning"] == 1
    return c["one_anchor"] == 0 and c["ref_spanning"] == 0


def _records(g, slow, rest):
    """(the P distinct records, which of them the kernel queues, which of them support an event)"""
    rng = random.Random(53)
    slow, rest = list(slow), list(rest)
    rng.shuffle(slow)
    rng.shuffle(rest)
    n_slow = len(slow)
    assert n_slow + len(rest) == P
    kinds = [slow.pop() if (j + 1) * n_slow // P > j * n_slow // P else rest.pop() for j in range(P)]   # the queued ones evenly spread
    recs, seen = [], set()
    for j, kd in enumerate(kinds):
        for _ in range(200):
            r = _draw(g, rng, kd, (L, R)[j % 2])                   # both sides in turn
            if r not in seen and "N" not in r and _is(g, r, kd):
                break
        else:
            raise AssertionError("no record of kind %s" % kd)
        seen.add(r)
        recs.append(r)
    return recs, np.array([kd in TALLY_OF for kd in kinds]), np.array([kd == "breakend" for kd in kinds])


MIXES = {"two_in_five": (["breakend"] * 30 + ["short"] * 4 + ["mismatched"] * 4 + ["hanging"] * 2, ["plain"] * 44 + ["deletion"] * 12 + ["foreign"] * 5),
         "all": (["breakend"] * 81 + ["short"] * 8 + ["mismatched"] * 8 + ["hanging"] * 4, [])}


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_two_and_a_half_trips_of_the_grid_in_one_push(mix):
    import torch
    seqs = breakend_cases.crafted_genome()
    g = breakends_ref.Genome([name for name, _ in seqs], [s for _, s in seqs], K)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * 8
    n = -(-5 * grid * 256 // 2)                                    # ceil(2.5 x CUs x 8 x 256)
    recs, queued, supporting = _records(g, *MIXES[mix])
    assert len(set(recs)) == P and all(len(r) == N_LEN for r in recs)
    q, rem = divmod(n, P)

    # the queue's paths, counted on the host before anything is pushed
    per_trip, drained, carried, left = _queue_walk(queued, n, grid)
    trips, waves = per_trip.shape
    assert trips == 3 and waves == grid * 4
    full = np.arange(trips)[:, None] * waves * 64 + np.arange(waves)[None, :] * 64 + 64 <= n
    three = full[2]                                                # the waves that go round three times
    assert three.sum() >= waves // 4
    if mix == "all":
        assert (per_trip[full] == 64).all() and drained[full].all()   # a full wave of waiting records on every trip: walked at once
        assert n % 64 == 0 and (left == 0).all()                   # ... and nothing remains for the kernel's end
    else:
        assert per_trip[full].min() >= 20 and per_trip[full].max() <= 45
        assert not drained[0].any()
        assert (drained[1, three] | drained[2, three]).all()       # ... cross 64 on their second or third trip
        assert (carried[1] > 0).all() and (carried[2, three] > 0).all()   # every later trip begins with records waiting
        assert (left > 0).all()                                    # every wave walks a remainder at the end

    a, b = breakends_ref.breakend_events(g, recs, C, M), breakends_ref.breakend_events(g, recs[:rem], C, M)
    both = breakends_ref.Result({key: [q * f + b.events.get(key, [0, 0])[0], q * r + b.events.get(key, [0, 0])[1]] for key, (f, r) in a.events.items()},
                                _scaled(a.span, b.span, q).tolist(), {name: q * a.counters[name] + b.counters[name] for name in a.counters})
    assert set(b.events) <= set(a.events) and len(a.events) >= 30
    assert all(v > 0 for name, v in a.counters.items() if name != "through" and (mix != "all" or name != "ref_spanning")), a.counters
    assert {key[1] for key in a.events} == {L, R} and min(sum(v[i] for v in a.events.values()) for i in (0, 1)) >= 5
    assert both.counters["supporting"] == int(supporting[np.arange(n) % P].sum()) <= int(queued[np.arange(n) % P].sum()) == both.counters["one_anchor"]

    words, lens = pack_reads([r.encode() for r in recs], K)
    assert words.shape == (P, 4) and (lens == N_LEN).all()
    idx = np.arange(n) % P
    ix = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in seqs])])
    eng = ix.engine()
    try:
        eng.breakends_enable(C, M)
        eng.sample_begin()
        eng.push_reads(0, words[idx], lens[idx])
        eng.sample_finalize(1)
        eng.sample_breakends(1)
        summ, rows = eng.download_breakends()
        want = breakends_ref.table_rows(g, both)
        assert rows == want, ([r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
        got = (summ.records, summ.one_anchor, summ.ref_spanning, summ.supporting, summ.short_, summ.through, summ.discordant, summ.unplaced)
        assert got == breakends_ref.counters_tuple(both) and summ.records == n
        assert summ.candidates == summ.reported == len(want) and summ.overflow == 0
        span = eng.download_breakend_span()
        sums = np.array(both.span_sums()[:g.cells], np.int64).astype(np.uint32)
        assert np.array_equal(span, sums), np.flatnonzero(span != sums)[:5]
    finally:
        eng.close()
        ix.close()
