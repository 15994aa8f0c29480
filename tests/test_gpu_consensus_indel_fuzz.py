"""The random cases of tests/consensus_indel_fuzz.py on the engine -- ci_best_kernel, ci_ties_kernel and ci_apply_kernel
(bk_consensus_indels.hip) on dense collisions made of reads, two samples in a row on one engine per case, each at seven (D, F) pairs:
the accepted rows, the nine tallies and the edited letters equal the restatements', bk_consensus_summary is untouched, overflow is 0.
Every comparison is exact.  tests/test_consensus_indel_fuzz_cpu.py runs the same iterations through the host twins and asserts what
they exercise.  Then the step's two refusals: more than BK_CONSENSUS_INDEL_MAX accepted events, and a full indel table."""
import numpy as np
import pytest

from bronko_amd import BronkoError, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import consensus_indel_fuzz as fuzz
from tests import consensus_indels_ref as ref
from tests import indels_ref

pytestmark = pytest.mark.gpu
MAX = 65536                                      # BK_CONSENSUS_INDEL_MAX


@pytest.mark.parametrize("block", range(fuzz.BLOCKS))
def test_engine_equals_the_restatement(block):
    ran, bad = fuzz.run(fuzz.SEED, block * fuzz.BLOCK, fuzz.BLOCK, fuzz.check_engine)
    assert ran == fuzz.BLOCK and not bad, "\n".join("%s: %s" % b for b in bad)


# ---- the two refusals -------------------------------------------------------------------------------------------------------------------
class Overflow:
    """fuzz.overflow_world(): 65,537 reads of 80 bases on a genome of 70,000 cells at k = 21, each its own one-base insertion with one
    supporting read (tests/test_consensus_indel_fuzz_cpu.py holds that against the restatement for the first 3,000)"""

    def __init__(self):
        self.names, self.seqs, self.reads, self.cells = fuzz.overflow_world()
        self.ix = HostIndex.build_mem(fuzz.OVERFLOW_K, [("overflow", [(n, s.encode()) for n, s in zip(self.names, self.seqs)])])
        self.n_cells = sum(len(s) for s in self.seqs)


@pytest.fixture(scope="module")
def overflow():
    w = Overflow()
    yield w
    w.ix.close()


def _to_call(eng, reads):
    """A sample of the reads (bytes) up to bk_sample_call; returns the whole indel table as bk_sample_indels(1, 0) reports it, a kernel
    of its own that tests/test_gpu_indels.py holds against the restatement"""
    eng.sample_begin()
    words, lens = pack_reads(reads, fuzz.OVERFLOW_K)
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_indels(1, 0)
    summ, report = eng.download_indels()
    assert summ.candidates == summ.reported == len(report) == len(reads) and summ.overflow == 0
    assert all(r[2] + r[3] == 1 and r[1] == -1 for r in report)              # every read its own insertion of one base
    eng.sample_call(1)
    return report


def small_dense_sample(seqs):
    """A dense read set of the fuzz in the first 700 cells of the overflow genome's second sequence"""
    return fuzz.dense_reads(np.random.default_rng([fuzz.SEED, 1]), fuzz.OVERFLOW_K, [seqs[1][:700]])[0]


def _tallies(summ):
    return {n: getattr(summ, n) for n in ref.TALLIES}


def _only_insertions(n, accepted):
    """The nine tallies of n candidates that are one-base insertions which share no boundary, `accepted` of them accepted"""
    return dict(candidates=n, accepted=accepted, applied=accepted, contested=0, deletions=0, insertions=accepted, deleted_bases=0, inserted_bases=accepted,
                frameshifts=accepted)


def _refused(eng):
    """The download of the current step is refused: (status, bk_last_error's text)"""
    with pytest.raises(BronkoError) as ei:
        eng.download_consensus_indels()
    return ei.value.status, eng._L.bk_last_error().decode()


def test_65536_accepted_events_travel_and_one_more_does_not(overflow):
    w = overflow
    assert len(w.reads) == MAX + 1
    eng = w.ix.engine()
    try:
        eng.indels_enable(32, 2, 20)                                         # 2^20 slots: the slot passes go round twice, and both trips append
        # BK_CONSENSUS_INDEL_MAX accepted events: every row arrives once
        report = _to_call(eng, w.reads[:MAX])
        plain, summ, rows, edited = fuzz.step(eng, 1, 0.0)
        assert summ.file_id == 0 and summ.overflow == 0 and _tallies(summ) == _only_insertions(MAX, MAX)
        want = fuzz.rows_of_report(report)
        assert len(rows) == MAX and rows == want, (len(rows), len(set(rows)), sorted(set(rows) - set(want))[:3], sorted(set(want) - set(rows))[:3])   # (both sorted: no hole, no duplicate)
        assert sorted(r[0] for r in rows) == sorted(w.cells[:MAX])
        assert edited == plain and len(plain) == w.n_cells and b"-" not in plain
        # one more: the download is an error, and says which
        _to_call(eng, w.reads)
        eng.sample_consensus(eng.consensus_params(min_depth=1, min_freq=0.0))
        eng.sample_consensus_indels()
        status, text = _refused(eng)
        assert status == -1 and "more than 65536 accepted events" in text, (status, text)
        # the flag and the rows are a call's: the same sample at thresholds that accept nothing ...
        plain, summ, rows, edited = fuzz.step(eng, 10, 0.5)
        assert summ.file_id == 0 and summ.overflow == 0 and _tallies(summ) == _only_insertions(MAX + 1, 0)
        assert rows == [] and edited == plain and b"-" not in plain
        # ... and a small dense sample behind it, against the restatement
        g = indels_ref.Genome(w.names, w.seqs, fuzz.OVERFLOW_K)
        dense = small_dense_sample(w.seqs)
        res = indels_ref.indel_events(g, dense)
        events, sums = ref.events_of(res), res.span_sums()
        assert len(events) >= 5 and all(g.seq_of(e[0]) == 1 for e in events)
        fuzz.sample_to_call(eng, dense, fuzz.OVERFLOW_K)
        seen = {}
        for D, F in ((1, 0.0), (10, 0.25)):
            rows, seen[D] = ref.resolve(events, sums, D, F)
            fuzz.check_step(eng, w.n_cells, rows, seen[D], D, F, "behind the overflow")
        assert seen[1]["contested"] >= 1 and seen[10]["applied"] >= 1
    finally:
        eng.close()


def test_a_full_indel_table_fails_this_download_too(overflow):
    w = overflow
    eng = w.ix.engine()
    try:
        eng.indels_enable(32, 2, 10)                                         # 2^10 slots and 1,500 distinct events
        eng.sample_begin()
        words, lens = pack_reads(w.reads[:1500], fuzz.OVERFLOW_K)
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        with pytest.raises(BronkoError) as ei:                               # (bk_sample_download_indels tells: test_gpu_indels.py)
            eng.download_indels()
        assert ei.value.status == -1
        eng.sample_call(1)
        eng.sample_consensus(eng.consensus_params(min_depth=1, min_freq=0.0))
        eng.sample_consensus_indels()                                        # returns; events were lost before this step, so its download fails
        status, text = _refused(eng)
        assert status == -1 and "a full indel event table" in text, (status, text)
        # the same call order with 600 of the reads: every one accepted and applied
        report = _to_call(eng, w.reads[:600])
        plain, summ, rows, edited = fuzz.step(eng, 1, 0.0)
        assert summ.file_id == 0 and summ.overflow == 0 and _tallies(summ) == _only_insertions(600, 600)
        assert rows == fuzz.rows_of_report(report) and sorted(r[0] for r in rows) == sorted(w.cells[:600])
        assert edited == plain and b"-" not in plain
    finally:
        eng.close()
