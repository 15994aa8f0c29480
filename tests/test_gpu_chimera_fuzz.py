"""Random records through bk_chimeras_enable: chimera_cases.fuzz_world at several seeds -- genomes of three to five sequences with
shared and reverse-complemented stretches and a run of N; reads that join two sequences in all four orientations, turn inside one,
carry deletions and errors --, each against tests/chimeras_ref.py at a drawn number of mismatches, through every push path, with one
or two mate files, in one push or several.  A few hundred records a seed, no case left out; the host twin is held against the same
cases without a GPU by the CPU half below."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import chimera_cases, chimeras_ref, rider_fuzz

SEEDS = (30411, 30412, 30413, 30414, 30415, 30416)
RECORDS = 400
KS = (21, 31, 15, 25)


def _case(seed):
    """(a case as rider_fuzz pushes one, max_mismatches, the restatement's result)"""
    rng = np.random.default_rng([seed, 9])
    seqs, reads = chimera_cases.fuzz_world(seed, RECORDS)
    k = int(KS[int(rng.integers(0, len(KS)))])
    M = int(rng.integers(0, 9))
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
    g = chimeras_ref.Genome([name for name, _ in seqs], [s for _, s in seqs], k)
    return case, M, g, seen, chimeras_ref.chimera_events(g, seen, M)


def _what(case, M):
    return "seed=%d k=%d M=%d push=%s batch=%s mates=%d" % (case.seed, case.k, M, case.push, case.batch, case.n_mates)


def _files(case):
    return [("fuzz", [(name, s.encode()) for name, s in case.seqs])]


def test_the_seeds_reach_every_tally_and_every_push_path():
    total = {name: 0 for name in chimeras_ref.TALLIES}
    sides, pushes, events = set(), set(), 0
    for seed in SEEDS:
        case, M, g, seen, res = _case(seed)
        for name, v in res.counters.items():
            total[name] += v
        sides |= {(key[1], key[3]) for key in res.events}
        events += len(res.events)
        pushes.add(case.push)
    assert all(v > 0 for v in total.values()), total
    assert len(sides) == 4 and events >= 300 and pushes == set(rider_fuzz.PUSHES)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_twin(seed):
    from bronko_amd import hostlib
    from bronko_amd.hostlib import HostIndex
    case, M, g, seen, res = _case(seed)
    ix = HostIndex.build_mem(case.k, _files(case))
    try:
        rows, span, counters = hostlib.chimera_events(ix, 0, seen, M)
        assert rows == chimeras_ref.table_rows(g, res), _what(case, M)
        assert np.array_equal(span, np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)), _what(case, M)
        assert counters == chimeras_ref.counters_tuple(res), _what(case, M)
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_engine(seed):
    from bronko_amd.hostlib import HostIndex
    case, M, g, seen, res = _case(seed)
    ix = HostIndex.build_mem(case.k, _files(case))
    eng = None
    try:
        eng = ix.engine()
        eng.chimeras_enable(M, 10)
        for _ in range(2 if case.twice else 1):
            rider_fuzz._sample(eng, case)
            eng.sample_chimeras(1)
            summ, rows = eng.download_chimeras()
            want = chimeras_ref.table_rows(g, res)
            assert rows == want, (_what(case, M), [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
            got = (summ.records, summ.same_strand, summ.ref_spanning, summ.crossed, summ.supporting, summ.discordant)
            assert got == chimeras_ref.counters_tuple(res), (_what(case, M), got, res.counters)
            assert (summ.candidates, summ.reported, summ.overflow) == (len(want), len(want), 0), _what(case, M)
            span = eng.download_chimera_span()
            sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
            assert np.array_equal(span, sums), (_what(case, M), np.flatnonzero(span != sums)[:5])
    finally:
        if eng is not None:
            eng.close()
        ix.close()
