"""Random records through bk_duplications_enable: tests/rider_fuzz.py's cases -- random genomes of one to three sequences with
repeats and runs of N, reads with deletions of 1 to 33 bases, chimeras of two places (forward and backward jumps of any length, the
arms anywhere in their sequence), foreign reads, errors, every push path, one or two mate files -- each against
tests/duplications_ref.py at a drawn min_len and number of mismatches.  A few hundred records a seed, no case left out; the host
twin is held against the same cases without a GPU by the CPU half below."""
import numpy as np
import pytest

from tests import duplications_ref, rider_fuzz

SEEDS = (20281, 20282, 20283, 20284, 20285)
RECORDS = 600                                    # a seed's cases are drawn until they hold this many reads
MIN_LENS = (1, 2, 20, 33, 33, 100)


def _cases(seed):
    """(case, min_len, max_mismatches, the restatement's result) for the seed's cases"""
    rng = np.random.default_rng([seed, 8])
    out, n, it = [], 0, 0
    while n < RECORDS:
        case = rider_fuzz.make_case(seed, it)
        it += 1
        if case is None:
            continue
        L, M = int(rng.choice(MIN_LENS)), int(rng.integers(0, 9))
        out.append((case, L, M, duplications_ref.duplication_events(case.genome(), case.reads_seen(), L, M)))
        n += len(case.reads)
    return out


def _what(case, L, M):
    return "%s duplication_L=%d duplication_M=%d" % (case.describe(), L, M)


def test_the_seeds_reach_every_tally():
    """What the cases exercise, counted from the restatement alone: every tally, at least 30 distinct events, on both strands, several min_len."""
    total = {name: 0 for name in duplications_ref.TALLIES}
    fwd = rev = events = 0
    lens = set()
    for seed in SEEDS:
        for case, L, M, res in _cases(seed):
            for name, v in res.counters.items():
                total[name] += v
            fwd += sum(e[0] for e in res.events.values())
            rev += sum(e[1] for e in res.events.values())
            events += len(res.events)
            lens.add(L)
    assert all(v > 0 for v in total.values()), total
    assert fwd > 0 and rev > 0 and events >= 30 and len(lens) >= 4


@pytest.mark.parametrize("seed", SEEDS)
def test_host_twin(seed):
    from bronko_amd import hostlib
    from bronko_amd.hostlib import HostIndex
    for case, L, M, res in _cases(seed):
        ix = HostIndex.build_mem(case.k, case.files())
        try:
            g = case.genome()
            rows, span, counters = hostlib.duplication_events(ix, 0, case.reads_seen(), L, M)
            assert rows == duplications_ref.table_rows(g, res), _what(case, L, M)
            assert np.array_equal(span, np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)), _what(case, L, M)
            assert counters == duplications_ref.counters_tuple(res), _what(case, L, M)
        finally:
            ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_engine(seed):
    from bronko_amd.hostlib import HostIndex
    for case, L, M, res in _cases(seed):
        ix = HostIndex.build_mem(case.k, case.files())
        eng = None
        try:
            eng = ix.engine()
            eng.duplications_enable(L, M, 10)
            g = case.genome()
            for _ in range(2 if case.twice else 1):
                rider_fuzz._sample(eng, case)
                eng.sample_duplications(1)
                summ, rows = eng.download_duplications()
                want = duplications_ref.table_rows(g, res)
                assert rows == want, (_what(case, L, M), [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
                got = (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.short_, summ.forward, summ.discordant)
                assert got == duplications_ref.counters_tuple(res), (_what(case, L, M), got, res.counters)
                assert (summ.candidates, summ.reported, summ.overflow) == (len(want), len(want), 0), _what(case, L, M)
                span = eng.download_duplication_span()
                sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
                assert np.array_equal(span, sums), (_what(case, L, M), np.flatnonzero(span != sums)[:5])
        finally:
            if eng is not None:
                eng.close()
            ix.close()
