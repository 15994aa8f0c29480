"""Random records through bk_breakends_enable: breakend_cases.fuzz_world at several seeds -- genomes of three to five sequences with a
repeat and a run of N; reads that leave the reference at shared sites, at the borders and at random cells with random, shared or
adapter bases, plain reads, deletions and foreign reads --, each against tests/breakends_ref.py at a drawn k, min_clip and number of
mismatches, through every push path, with one or two mate files, in one push or several.  A few hundred records a seed, no case
left out; the host twin is held against the same cases without a GPU by the CPU half below."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import breakend_cases, breakends_ref, rider_fuzz
from tests.breakends_ref import L, R

SEEDS = (41511, 41512, 41513, 41514, 41515, 41516)
RECORDS = 400
KS = (21, 31, 15, 25)


def _case(seed):
    """(a case as rider_fuzz pushes one, min_clip, max_mismatches, the restatement's result)"""
    rng = np.random.default_rng([seed, 11])
    k = int(KS[seed % len(KS)])                                     # every k among the seeds
    seqs, reads = breakend_cases.fuzz_world(seed, RECORDS, k)
    M = int(rng.integers(0, 9))
    C = int(rng.choice((16, 17, 20, 25, 40)))
    push = rider_fuzz.PUSHES[seed % len(rider_fuzz.PUSHES)]        # every path among the seeds
    reads = [r.encode() for r in reads]
    quals = [b"I" * len(r) for r in reads]
    for i in rng.integers(0, len(reads), 40):                       # a base of low quality: under ascii_qual the read is two records
        qv = bytearray(quals[i])
        qv[int(rng.integers(0, len(qv)))] = 33 + 7
        quals[i] = bytes(qv)
    case = SimpleNamespace(seed=seed, k=k, reads=reads, quals=quals, push=push, trim=False, batch=int(rng.integers(30, 200)) if rng.random() < 0.5 else None,
                           n_mates=2 if rng.random() < 0.5 else 1, twice=bool(rng.random() < 0.5), seqs=seqs)
    case.mates = lambda: [(0, len(reads))] if case.n_mates == 1 else [(0, len(reads) // 2), (len(reads) // 2, len(reads))]
    from tests import adapter_ref
    seen = [r.decode() for r in adapter_ref.masked(reads, quals, rider_fuzz.MIN_QUAL if push == "ascii_qual" else 0)]
    g = breakends_ref.Genome([name for name, _ in seqs], [s for _, s in seqs], k)
    return case, C, M, g, seen, breakends_ref.breakend_events(g, seen, C, M)


def _what(case, C, M):
    return "seed=%d k=%d C=%d M=%d push=%s batch=%s mates=%d" % (case.seed, case.k, C, M, case.push, case.batch, case.n_mates)


def _files(case):
    return [("fuzz", [(name, s.encode()) for name, s in case.seqs])]


def test_the_seeds_reach_every_tally_every_k_and_every_push_path():
    total = {name: 0 for name in breakends_ref.TALLIES}
    sides, pushes, ks, events, strands = set(), set(), set(), 0, [0, 0]
    for seed in SEEDS:
        case, C, M, g, seen, res = _case(seed)
        for name, v in res.counters.items():
            total[name] += v
        sides |= {key[1] for key in res.events}
        events += len(res.events)
        strands = [strands[0] + sum(f for f, r in res.events.values()), strands[1] + sum(r for f, r in res.events.values())]
        pushes.add(case.push)
        ks.add(case.k)
    assert all(v > 0 for v in total.values()), total
    assert sides == {L, R} and events >= 150 and min(strands) >= 100 and pushes == set(rider_fuzz.PUSHES) and ks == set(KS)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_twin(seed):
    from bronko_amd import hostlib
    from bronko_amd.hostlib import HostIndex
    case, C, M, g, seen, res = _case(seed)
    ix = HostIndex.build_mem(case.k, _files(case))
    try:
        rows, span, counters = hostlib.breakend_events(ix, 0, seen, C, M)
        assert rows == breakends_ref.table_rows(g, res), _what(case, C, M)
        assert np.array_equal(span, np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)), _what(case, C, M)
        assert counters == breakends_ref.counters_tuple(res), _what(case, C, M)
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_engine(seed):
    from bronko_amd.hostlib import HostIndex
    case, C, M, g, seen, res = _case(seed)
    ix = HostIndex.build_mem(case.k, _files(case))
    eng = None
    try:
        eng = ix.engine()
        eng.breakends_enable(C, M, 10)
        for _ in range(2 if case.twice else 1):
            rider_fuzz._sample(eng, case)
            eng.sample_breakends(1)
            summ, rows = eng.download_breakends()
            want = breakends_ref.table_rows(g, res)
            assert rows == want, (_what(case, C, M), [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
            got = (summ.records, summ.one_anchor, summ.ref_spanning, summ.supporting, summ.short_, summ.through, summ.discordant, summ.unplaced)
            assert got == breakends_ref.counters_tuple(res), (_what(case, C, M), got, res.counters)
            assert (summ.candidates, summ.reported, summ.overflow) == (len(want), len(want), 0), _what(case, C, M)
            span = eng.download_breakend_span()
            sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
            assert np.array_equal(span, sums), (_what(case, C, M), np.flatnonzero(span != sums)[:5])
    finally:
        if eng is not None:
            eng.close()
        ix.close()
