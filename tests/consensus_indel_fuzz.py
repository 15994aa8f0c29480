"""Random cases for bk_sample_consensus_indels (bk_consensus_indels.hip) and its host twin (bh_consensus_indels): dense collisions
made of reads.

make_case(seed, iteration) draws one case -- k, one genome file of one to three random sequences, the indel table's size, the
mismatch limit and TWO read sets that run in a row on one engine -- from numpy's generator seeded with (seed, iteration); nothing else
goes in.  A dense read set is tests/test_consensus_indels_cpu.py's _random_events made of reads: 2 to 40 events drawn in a cluster of
12, 60 or 200 cells, each written as 1 to 30 reads of 150 bases (indel_cases.mut_read) with the breakpoint at a drawn offset, either
strand, and 0 to 40 plain reads over the cluster as span.  The events are not predicted: left-normalisation and the anchor rule decide
them, and expected(case) asks the restatements alone -- tests/indels_ref.py for reads -> events and span,
tests/consensus_indels_ref.py for the rule at every pair of PAIRS.  check_host holds the host twins (bronko_amd.hostlib) against that,
check_engine the engine; they are the only functions that import the product.  tally() counts what a run of cases has exercised, for
the conditions of tests/test_consensus_indel_fuzz_cpu.py.  tests/test_gpu_consensus_indel_fuzz.py runs the same cases.

overflow_world() is the input of the two overflow tests: a genome of 70,000 cells and one read per drawn cell, each of which makes
its own one-base insertion with one supporting read.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import consensus_indels_ref as ref
from tests import indel_cases, indels_ref
from tests.indels_ref import DEL, INS

B = "ACGT"
KS = (15, 21, 21, 31)
TABLE_LOG2 = (10, 12, 16)
MAX_MISMATCHES = (0, 2)
WIDTHS = (12, 60, 200)
LENGTHS = (1, 1, 2, 3, 3, 4, 6, 9, 17, 32)
SUPPORTS = (1, 2, 5, 5, 10, 10, 11, 30)
PLAIN = (0, 0, 3, 10, 40)
SECOND = ("dense", "dense", "sparse", "empty")
MAX_LEN = 32                                     # bk_indels_enable's max_len in every case
N = indel_cases.N_LEN                            # 150 bases a read
MARGIN = 130                                     # a cluster keeps so many cells from its sequence's ends
# the pairs every sample is checked at: the tests' four, and three whose F is no double's exact fraction while F * n is the integer
# itself where the fraction's is one (1/3 * 3.0 is 1.0, 0.1 * 20.0 is 2.0, 0.7 * 10.0 is 7.0): s on it is accepted, s below it is not
PAIRS = ref.PAIRS + ((3, 1 / 3), (2, 0.1), (5, 0.7))
SEED = 20262                                     # the suite's seed
BLOCK, BLOCKS = 10, 4                            # the suite's iterations: BLOCKS blocks of BLOCK
TALLIES5 = ("positions", "called", "ambiguous", "masked", "substitutions")


def rand_seq(rng, n: int) -> str:
    return "".join(B[i] for i in rng.integers(0, 4, n))


@dataclass
class Case:
    seed: int
    it: int
    k: int
    names: list
    seqs: list
    table_log2: int
    max_mismatches: int
    kinds: tuple                     # of the two read sets: "dense", "sparse" or "empty"
    samples: list                    # the two read sets: [str]
    drawn: list                      # per sample: how many events were drawn, before the rule has its say
    clusters: list                   # per sample: (sequence, first cell in it, width) or None

    def files(self):
        return [("fuzz", [(name, s.encode()) for name, s in zip(self.names, self.seqs)])]

    def genome(self) -> indels_ref.Genome:
        return indels_ref.Genome(list(self.names), list(self.seqs), self.k)

    def describe(self) -> str:
        return ("seed=%d it=%d k=%d seqs=%s table_log2=%d max_mismatches=%d samples=%s reads=%s drawn=%s clusters=%s" %
                (self.seed, self.it, self.k, [len(s) for s in self.seqs], self.table_log2, self.max_mismatches, "+".join(self.kinds),
                 [len(r) for r in self.samples], self.drawn, self.clusters))


def _strand(rng, r: str) -> str:
    return indels_ref.revcomp(r) if rng.random() < 0.5 else r


def _plain(rng, text: str, lo: int, width: int, n: int) -> list:
    """n reads of the sequence as it is, each over a part of the cluster [lo, lo + width)"""
    return [_strand(rng, text[a:a + N]) for a in (int(rng.integers(lo - 120, lo + width - 29)) for _ in range(n))]


def dense_reads(rng, k: int, seqs: list):
    """(reads, events drawn, (sequence, first cell, width)): see the module's text.  The read of an event at `cell` starts at
    cell - p; p leaves more than k + 4 bases of the reference at both ends of the read and keeps the read inside the sequence."""
    q = int(rng.integers(0, len(seqs)))
    text = seqs[q]
    width = int(rng.choice([w for w in WIDTHS if w <= len(text) - 2 * MARGIN]))
    lo = int(rng.integers(MARGIN, len(text) - MARGIN - width + 1))
    reads = []
    n_events = int(rng.integers(2, 41))
    for _ in range(n_events):
        cell = lo + int(rng.integers(0, width))
        kind = int(rng.choice([DEL, INS]))
        length = int(rng.choice(LENGTHS))
        S = rand_seq(rng, length) if kind == INS else ""
        support = int(rng.choice(SUPPORTS))
        p_lo = max(k + 5, cell + N + length - len(text)) if kind == DEL else k + 5
        p_hi = N - k - 5 - (length if kind == INS else 0)
        for _ in range(support):
            p = int(rng.integers(p_lo, p_hi + 1))
            subs = (int(rng.integers(0, N)),) if rng.random() < 0.05 else ()   # now and then a substitution: a mismatch, or a lost anchor
            r = indel_cases.mut_read(text, cell - p, N, dele=(cell, length) if kind == DEL else None, ins=(cell, S) if kind == INS else None, subs=subs)
            reads.append(_strand(rng, r))
    reads += _plain(rng, text, lo, width, int(rng.choice(PLAIN)))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], n_events, (q, lo, width)


def _sparse(rng, k: int, seqs: list):
    """A few events of one read each anywhere in one sequence, and plain reads between them"""
    q = int(rng.integers(0, len(seqs)))
    text = seqs[q]
    reads = []
    n_events = int(rng.integers(1, 5))
    for _ in range(n_events):
        length = int(rng.choice(LENGTHS))
        cell = int(rng.integers(MARGIN, len(text) - MARGIN))
        p = int(rng.integers(max(k + 5, cell + N + length - len(text)), N - k - 5 - length + 1))
        if rng.random() < 0.5:
            r = indel_cases.mut_read(text, cell - p, N, dele=(cell, length))
        else:
            r = indel_cases.mut_read(text, cell - p, N, ins=(cell, rand_seq(rng, length)))
        reads.append(_strand(rng, r))
    reads += [_strand(rng, text[a:a + N]) for a in (int(rng.integers(0, len(text) - N + 1)) for _ in range(int(rng.integers(5, 30))))]
    return reads, n_events, None


def _empty(rng, k: int, seqs: list):
    """Plain reads alone: the sample selects the genome and has no event"""
    text = seqs[int(rng.integers(0, len(seqs)))]
    return [_strand(rng, text[a:a + N]) for a in (int(rng.integers(0, len(text) - N + 1)) for _ in range(int(rng.integers(5, 40))))], 0, None


def make_case(seed: int, it: int) -> Case:
    rng = np.random.default_rng([seed, it])
    k = int(rng.choice(KS))
    seqs = [rand_seq(rng, int(rng.integers(300, 901))) for _ in range(int(rng.integers(1, 4)))]
    table_log2 = int(rng.choice(TABLE_LOG2))
    max_mismatches = int(rng.choice(MAX_MISMATCHES))
    kinds = ("dense", str(rng.choice(SECOND)))
    made = [dict(dense=dense_reads, sparse=_sparse, empty=_empty)[kind](rng, k, seqs) for kind in kinds]
    return Case(seed=seed, it=it, k=k, names=["s%d" % i for i in range(len(seqs))], seqs=seqs, table_log2=table_log2, max_mismatches=max_mismatches,
                kinds=kinds, samples=[m[0] for m in made], drawn=[m[1] for m in made], clusters=[m[2] for m in made])


@dataclass
class Sample:
    res: indels_ref.Result
    events: list                     # [(cell, kind, length, S, s)]
    sums: list                       # the prefix-summed span array
    resolved: dict = field(default_factory=dict)      # {(D, F): (rows, tallies)} of ref.resolve


@dataclass
class Expected:
    g: indels_ref.Genome
    samples: list


def expected(case: Case) -> Expected:
    """The restatements' results of the case's two samples at every pair"""
    g = case.genome()
    out = []
    for reads in case.samples:
        res = indels_ref.indel_events(g, reads, MAX_LEN, case.max_mismatches)
        assert len(res.events) <= 1 << case.table_log2
        s = Sample(res, ref.events_of(res), res.span_sums())
        for D, F in PAIRS:
            s.resolved[(D, F)] = ref.resolve(s.events, s.sums, D, F)
        out.append(s)
    return Expected(g, out)


def _share(x, y) -> bool:
    a, b = ref.occupied(x[0], x[1], x[2]), ref.occupied(y[0], y[1], y[2])
    return a.start < b.stop and b.start < a.stop


def tally(case: Case, exp: Expected, into: dict) -> dict:
    """What the case exercised, from the restatements' results alone, added into `into`.  A pair of events counts once per (D, F) at
    which both are accepted; an event once per (D, F)."""
    def add(name, v=1):
        into[name] = into.get(name, 0) + int(v)
    add("iterations")
    add("k=%d" % case.k)
    for i, s in enumerate(exp.samples):
        add("samples")
        add("events", len(s.events))
        add("events_in_a_later_sequence", sum(1 for e in s.events if exp.g.seq_of(e[0]) > 0))
        most = max(t["accepted"] for _, t in s.resolved.values())
        add("samples_20_accepted", most >= 20)
        into["largest_accepted_set"] = max(into.get("largest_accepted_set", 0), most)
        if i == 1:
            add("second_without_an_event", not s.events and len(exp.samples[0].events) >= 2)
        for (D, F), (rows, t) in s.resolved.items():
            add("applied", t["applied"])
            add("contested", t["contested"])
            add("rejected", t["candidates"] - t["accepted"])
            add("n_eq_D", sum(1 for e in s.events if e[4] + s.sums[e[0]] == D))
            if F > 0:
                add("exact_product", sum(1 for e in s.events if float(e[4]) == F * float(e[4] + s.sums[e[0]])))
            beaters = {j: [] for j in range(len(rows))}
            for j, x in enumerate(rows):
                for m, y in enumerate(rows):
                    if m == j or not _share(x, y):
                        continue
                    if not x[4] > y[4]:
                        beaters[j].append(m)
                    if m > j:
                        add("equal_support_pairs", x[4] == y[4])
                        if x[1] != y[1]:
                            ins, dele = (x, y) if x[1] == INS else (y, x)
                            add("ins_del_pairs")
                            add("ins_at_a_deletions_edge", ins[0] in (dele[0], dele[0] + dele[2]))
            for j, x in enumerate(rows):
                assert x[6] == (not beaters[j])                     # (the rule, said once more)
                add("contested_by_contested_only", bool(beaters[j]) and all(not rows[m][6] for m in beaters[j]))
            add("boundaries_shared_by_5", _crowded(rows, 5))
    return into


def _crowded(rows, n: int) -> int:
    """How many boundaries at least n accepted events occupy"""
    count = {}
    for x in rows:
        for b in ref.occupied(x[0], x[1], x[2]):
            count[b] = count.get(b, 0) + 1
    return sum(1 for v in count.values() if v >= n)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _differ(got, want):
    return [x for x in got if x not in want][:3], [x for x in want if x not in got][:3]


def check_host(case: Case, exp: Expected) -> None:
    """hostlib.indel_events -> hostlib.consensus_indels on both samples at every pair against the restatements; AssertionError names
    what differs.  The letters are the reference's own (any letters do)."""
    from bronko_amd import hostlib
    ix = hostlib.HostIndex.build_mem(case.k, case.files())
    letters = exp.g.text.encode()
    try:
        for i, (reads, s) in enumerate(zip(case.samples, exp.samples)):
            table, span, counters = hostlib.indel_events(ix, 0, reads, MAX_LEN, case.max_mismatches)
            want = indels_ref.table_rows(exp.g, s.res)
            assert table == want, ("sample %d: indel events" % i,) + _differ(table, want)
            want = np.array(s.sums[:exp.g.cells], np.int64).astype(np.uint32)
            assert np.array_equal(span, want), ("sample %d: indel span" % i, np.flatnonzero(span != want)[:5])
            for (D, F), (rows, t) in s.resolved.items():
                what = "sample %d at D = %d, F = %r" % (i, D, F)
                got_rows, got_t, got_letters = hostlib.consensus_indels(ix, 0, table, span, letters, D, F)
                assert got_rows == ref.abi_rows(rows), (what, "rows") + _differ(got_rows, ref.abi_rows(rows))
                assert got_t == t, (what, "tallies", got_t, t)
                assert got_letters == ref.edit_letters(letters, rows), (what, "letters")
    finally:
        ix.close()


def sample_to_call(eng, reads, k: int) -> None:
    """A sample of the reads (str) up to bk_sample_call, with the whole indel table reported"""
    from bronko_amd import pack_reads
    eng.sample_begin()
    words, lens = pack_reads([r.encode() for r in reads], k)
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_indels(1, 0)
    eng.sample_call(1)


def step(eng, D: int, F: float):
    """bk_sample_consensus at (D, F) and the step behind it: (plain letters, summary, rows, edited letters); bk_consensus_summary's
    five tallies stay those of the unedited letters"""
    eng.sample_consensus(eng.consensus_params(min_depth=D, min_freq=F))
    before, plain = eng.download_consensus()
    eng.sample_consensus_indels()
    summ, rows = eng.download_consensus_indels()
    after, edited = eng.download_consensus()
    assert [getattr(before, n) for n in TALLIES5] == [getattr(after, n) for n in TALLIES5] and before.file_id == after.file_id, "bk_consensus_summary changed"
    return plain, summ, rows, edited


def check_step(eng, cells: int, rows, t, D: int, F: float, what: str) -> None:
    """One step of the engine's current sample against the restatement's (rows, tallies) of it"""
    plain, summ, got, edited = step(eng, D, F)
    what = "%s at D = %d, F = %r" % (what, D, F)
    assert summ.file_id == 0 and summ.overflow == 0 and len(plain) == cells and b"-" not in plain, (what, summ.file_id, summ.overflow, len(plain))
    assert got == ref.abi_rows(rows), (what, "rows") + _differ(got, ref.abi_rows(rows))
    got_t = {n: getattr(summ, n) for n in ref.TALLIES}
    assert got_t == t, (what, "tallies", got_t, t)
    want = ref.edit_letters(plain, rows)
    if edited != want:
        bad = [c for c in range(len(plain)) if edited[c:c + 1] != want[c:c + 1]]
        raise AssertionError((what, "%d letters differ, first at %d" % (len(bad), bad[0])))


def check_engine(case: Case, exp: Expected) -> None:
    """One engine for the case: create, enable, the two samples in a row, each at every pair, close.  Whatever the first sample left
    in best, ties, the rows or the letters would show in the second."""
    from bronko_amd.hostlib import HostIndex
    ix = HostIndex.build_mem(case.k, case.files())
    eng = None
    try:
        eng = ix.engine()
        eng.indels_enable(MAX_LEN, case.max_mismatches, case.table_log2)
        for i, (reads, s) in enumerate(zip(case.samples, exp.samples)):
            sample_to_call(eng, reads, case.k)
            for (D, F), (rows, t) in s.resolved.items():
                check_step(eng, exp.g.cells, rows, t, D, F, "sample %d" % i)
    finally:
        if eng is not None:
            eng.close()
        ix.close()


def run(seed: int, first: int, count: int, check, out=print) -> tuple:
    """Cases first .. first + count - 1 of `seed` through `check` (check_host or check_engine): (cases run, [(case's line, message)])"""
    bad = []
    for it in range(first, first + count):
        case = make_case(seed, it)
        exp = expected(case)
        try:
            check(case, exp)
        except AssertionError as e:
            bad.append((case.describe(), str(e)[:400]))
            out("MISMATCH %s: %s" % bad[-1])
    return count, bad


# ---- the overflow tests' input --------------------------------------------------------------------------------------------------------
OVERFLOW_K = 21
OVERFLOW_SEQS = (30000, 25000, 15000)
OVERFLOW_READS = 65537                           # BK_CONSENSUS_INDEL_MAX + 1
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def overflow_world(seed: int = SEED):
    """(names, seqs, reads as bytes, cells): random sequences of OVERFLOW_SEQS cells and OVERFLOW_READS distinct cells in a drawn
    order, each at least 41 from its sequence's ends; the read of cell c is text[c-40:c] + X + text[c:c+39] with X another base than
    text[c-1] -- an insertion that cannot slide to the left --, every second one in the mean reverse-complemented.  (41 and not 40:
    the rule lays an insertion's read along the reference from its back anchor too, one cell further left, and refuses a read that
    leaves its sequence there -- the read of a sequence's cell 40 makes no event.)"""
    rng = np.random.default_rng([seed, 65537])
    seqs = [rand_seq(rng, n) for n in OVERFLOW_SEQS]
    text = "".join(seqs)
    ok, first = [], 0
    for s in seqs:
        ok.append(np.arange(first + 41, first + len(s) - 41 + 1))
        first += len(s)
    cells = [int(c) for c in rng.permutation(np.concatenate(ok))[:OVERFLOW_READS]]
    shift, rc = rng.integers(1, 4, len(cells)), rng.random(len(cells)) < 0.5
    reads = []
    for c, d, back in zip(cells, shift, rc):
        r = (text[c - 40:c] + B[(B.index(text[c - 1]) + int(d)) & 3] + text[c:c + 39]).encode()
        reads.append(r.translate(_RC)[::-1] if back else r)
    return ["o%d" % i for i in range(len(seqs))], seqs, reads, cells


def rows_of_report(report) -> list:
    """download_indels' rows (cell, len, fwd, rev, ref_span, seq) as the accepted and applied rows of the step: (cell, len, fwd + rev,
    ref_span, seq, 1)"""
    return [(c, ln, f + r, rs, sq, 1) for c, ln, f, r, rs, sq in report]
