"""The random cases of tests/consensus_indel_fuzz.py without a GPU: the host twins (hostlib.indel_events -> hostlib.consensus_indels)
against the Python restatements over the very iterations that tests/test_gpu_consensus_indel_fuzz.py runs on the engine -- both
samples of a case at every (D, F) pair: every accepted event with its status, the nine tallies, the edited letters.  Then the
conditions that keep the fuzz from being vacuous, asserted on the restatements' results alone and summed over those iterations, and
the premise of the GPU file's overflow tests: each of their reads makes its own one-base insertion."""
import functools

import pytest

from tests import consensus_indel_fuzz as fuzz
from tests import consensus_indels_ref as ref
from tests import indels_ref


@functools.lru_cache(maxsize=None)
def _case(it):
    case = fuzz.make_case(fuzz.SEED, it)
    return case, fuzz.expected(case)


@pytest.mark.parametrize("block", range(fuzz.BLOCKS))
def test_host_twins_equal_the_restatements(block):
    bad = []
    for it in range(block * fuzz.BLOCK, (block + 1) * fuzz.BLOCK):
        case, exp = _case(it)
        try:
            fuzz.check_host(case, exp)
        except AssertionError as e:
            bad.append("%s: %s" % (case.describe(), str(e)[:400]))
    assert not bad, "\n".join(bad)


def test_a_case_is_a_function_of_seed_and_iteration():
    a, b = fuzz.make_case(7, 3), fuzz.make_case(7, 3)
    assert a.describe() == b.describe() and a.samples == b.samples and a.seqs == b.seqs
    assert fuzz.make_case(7, 4).samples != a.samples and fuzz.make_case(8, 3).samples != a.samples
    assert a.k in fuzz.KS and a.table_log2 in fuzz.TABLE_LOG2 and a.max_mismatches in fuzz.MAX_MISMATCHES
    assert 1 <= len(a.seqs) <= 3 and all(300 <= len(s) <= 900 for s in a.seqs)
    assert len(a.samples) == 2 and a.kinds[0] == "dense" and a.kinds[1] in fuzz.SECOND
    assert all(len(r) == fuzz.N for reads in a.samples for r in reads)
    q, lo, width = a.clusters[0]
    assert width in fuzz.WIDTHS and lo >= fuzz.MARGIN and lo + width <= len(a.seqs[q]) - fuzz.MARGIN


def test_the_fuzz_is_not_vacuous():
    t = {}
    for it in range(fuzz.BLOCKS * fuzz.BLOCK):
        fuzz.tally(*_case(it), t)
    print(sorted(t.items()))
    # summed over all samples and pairs: what the three kernels were written to handle
    floors = dict(applied=300, contested=300, rejected=300,
                  equal_support_pairs=200,               # ties[b] == 2 with equal support
                  ins_del_pairs=200,                     # insertions on a deletion's boundaries
                  contested_by_contested_only=100,       # the one-round chain and the tie
                  n_eq_D=50, exact_product=50,           # both compares on their thresholds
                  samples_20_accepted=10,                # a wave's ballot with many accepted lanes, an append of many rows
                  second_without_an_event=5,             # stale best / ties / rows of a denser sample would show
                  events_in_a_later_sequence=1)
    # ... and what the list above does not say by itself
    floors.update(ins_at_a_deletions_edge=50, boundaries_shared_by_5=200, largest_accepted_set=30)
    floors.update({"k=%d" % k: 3 for k in set(fuzz.KS)})
    short = {name: (t.get(name, 0), floor) for name, floor in floors.items() if t.get(name, 0) < floor}
    assert not short, short


def test_the_extra_pairs_lie_on_ties():
    """What the three pairs behind ref.PAIRS are there for: none of the three F is a double's exact fraction, and yet the double
    product F * n is the integer itself at every n where the fraction's is one -- there s == F * n is accepted, s one less is not"""
    assert fuzz.PAIRS[:4] == ref.PAIRS and len(fuzz.PAIRS) == 7
    for F, step, share in ((1 / 3, 3, 1), (0.1, 10, 1), (0.7, 10, 7)):
        for m in range(1, 8):
            n, s = step * m, share * m
            assert F * float(n) == float(s) and ref.is_accepted(s, n - s, 1, F) and not ref.is_accepted(s - 1, n - s + 1, 1, F), (F, n)


def test_every_overflow_read_makes_its_own_insertion():
    """The first 3,000 reads of overflow_world(): by the restatement each makes exactly its own event (c, INS, 1, X) with one
    supporting read and no spanning one, and at (1, 0.0) all are accepted and applied, none contested.  The restatement is too slow
    for the 65,537; of those the host twin of the indel pass says the same, and the GPU tests ask the engine's own indel report."""
    names, seqs, reads, cells = fuzz.overflow_world()
    assert [len(s) for s in seqs] == list(fuzz.OVERFLOW_SEQS) and len(reads) == len(cells) == len(set(cells)) == fuzz.OVERFLOW_READS == 65537
    assert all(len(r) == 80 for r in reads)
    g = indels_ref.Genome(names, seqs, fuzz.OVERFLOW_K)
    for c in cells:
        q = g.seq_of(c)
        assert g.first[q] + 41 <= c <= g.first[q] + len(seqs[q]) - 41
    n = 3000
    res = indels_ref.indel_events(g, [r.decode() for r in reads[:n]])
    assert len(res.events) == n and res.counters["supporting"] == n and res.counters["ref_spanning"] == 0
    assert sorted(e[0] for e in res.events) == sorted(cells[:n])
    both = 0
    for (cell, kind, length, S), (fwd, rev) in res.events.items():
        assert (kind, length) == (indels_ref.INS, 1) and fwd + rev == 1 and S != g.text[cell - 1]
        both += rev
    assert n // 3 < both < 2 * n // 3                                              # either strand
    # at (1, 0.0) every one is accepted, and no two share a boundary: an insertion occupies its cell's alone, and the cells differ.  So
    # all are applied; ref.resolve, quadratic in the events, says so of the first 400.
    events, sums = ref.events_of(res), res.span_sums()
    assert all(ref.is_accepted(e[4], sums[e[0]], 1, 0.0) and not ref.is_accepted(e[4], sums[e[0]], 10, 0.5) for e in events)
    assert len({b for e in events for b in ref.occupied(e[0], e[1], e[2])}) == n
    m = 400
    rows, t = ref.resolve(events[:m], sums, 1, 0.0)
    assert t == dict(candidates=m, accepted=m, applied=m, contested=0, deletions=0, insertions=m, deleted_bases=0, inserted_bases=m, frameshifts=m)
    # all of them through the host twin (indels.cpp), which tests/test_indels_cpu.py holds against the restatement
    from bronko_amd import hostlib
    ix = hostlib.HostIndex.build_mem(fuzz.OVERFLOW_K, [("overflow", [(name, s.encode()) for name, s in zip(names, seqs)])])
    try:
        table, span, counters = hostlib.indel_events(ix, 0, [r.decode() for r in reads])
    finally:
        ix.close()
    assert [r[0] for r in table] == sorted(cells) and all(r[1] == -1 and r[2] + r[3] == 1 and r[4] == 0 for r in table) and not span.any()
