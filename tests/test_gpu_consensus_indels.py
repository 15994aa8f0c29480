"""bk_sample_consensus_indels (bk_consensus_indels.hip) against the Python restatement of the rule (tests/consensus_indels_ref.py).
The reference side is the restatement applied to indels_ref's events of the same reads and to the engine's own plain letters,
downloaded before the step: the accepted records as a set, every tally and the edited letters must be equal -- the rule is integer
arithmetic but for one product, no case is left out.  Then the slot passes' second grid trip, samples in a row, the C ABI's call
order, and `bronko call --consensus-indels` end to end."""
import gzip
import os
import random
import subprocess

import pytest

from bronko_amd import BronkoError, hostlib, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import consensus_indels_ref as ref
from tests import indel_cases, indels_ref
from tests.indels_ref import DEL, INS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21
N = indel_cases.N_LEN


def crafted_sample():
    """About 200 reads of 150 bases on crafted_genome(21), both strands: a 3-base deletion with 30 supporting and 10 spanning reads and
    a 2-base insertion with exactly 12 and 12 in the first sequence; in the second an event below D = 10 (3 and 2) and two overlapping
    deletions with 20 and 8 reads under the same 10 spanning reads; the rest plain reads that span none of them.  Returns (reads,
    the events as planted: {name: (cell, kind, length, S)})."""
    (_, a), (_, b) = indel_cases.crafted_genome(K)
    first_b = len(a)
    rng = random.Random(5)
    reads, planted = [], {}

    def add(text, starts, dele=None, ins=None):
        for i, st in enumerate(starts):
            r = indel_cases.mut_read(text, st, N, dele=dele, ins=ins)
            reads.append(indels_ref.revcomp(r) if i % 2 else r)

    p = indel_cases._free_pos(a, 800, 3)
    add(a, [p - 100 + 2 * i for i in range(30)], dele=(p, 3))
    add(a, [p - 90 + 3 * i for i in range(10)])
    planted["del3"] = (p, DEL, 3, "")
    p = indel_cases._free_pos(a, 960, 1)
    s = indel_cases._ins_seq(rng, a, p, 2)
    add(a, [p - 95 + 3 * i for i in range(12)], ins=(p, s))
    add(a, [p - 92 + 3 * i for i in range(12)])
    planted["ins2"] = (p, INS, 2, s)
    p = indel_cases._free_pos(b, 150, 4)
    add(b, [p - 80 + 5 * i for i in range(3)], dele=(p, 4))
    add(b, [p - 70 + 5 * i for i in range(2)])
    planted["below_D"] = (first_b + p, DEL, 4, "")
    p = indel_cases._free_pos(b, 450, 6)
    q = indel_cases._free_pos(b, p + 3, 5)
    assert q <= p + 6                                                # the two share a boundary
    add(b, [p - 100 + 2 * i for i in range(20)], dele=(p, 6))
    add(b, [p - 98 + 5 * i for i in range(8)], dele=(q, 5))
    add(b, [p - 90 + 3 * i for i in range(10)])
    planted["del6"], planted["del5"] = (first_b + p, DEL, 6, ""), (first_b + q, DEL, 5, "")
    add(a, [rng.randrange(1321, 1350) for _ in range(45)])           # plain reads that reach none of the events
    add(b, [rng.randrange(480, len(b) - N) for _ in range(44)])
    return reads, planted


class Crafted:
    def __init__(self):
        self.seqs = indel_cases.crafted_genome(K)
        self.ix = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in self.seqs])])
        self.g = indels_ref.Genome([name.split()[0] for name, _ in self.seqs], [s for _, s in self.seqs], K)
        self.reads, self.planted = crafted_sample()
        assert 190 <= len(self.reads) <= 210
        self.res = indels_ref.indel_events(self.g, self.reads)
        self.events, self.sums = ref.events_of(self.res), self.res.span_sums()
        # the case is what it is meant to be, by the restatement alone
        by = {e[:4]: (e[4], self.sums[e[0]]) for e in self.events}
        assert by[self.planted["del3"]] == (30, 10) and by[self.planted["ins2"]] == (12, 12) and by[self.planted["below_D"]] == (3, 2)
        assert by[self.planted["del6"]] == (20, 10) and by[self.planted["del5"]] == (8, 10)
        st = {r[:4]: r[6] for r in ref.resolve(self.events, self.sums, 10, 0.5)[0]}
        assert st[self.planted["del3"]] and st[self.planted["ins2"]] and st[self.planted["del6"]] and self.planted["del5"] not in st and self.planted["below_D"] not in st
        st = {r[:4]: r[6] for r in ref.resolve(self.events, self.sums, 10, 0.25)[0]}
        assert st[self.planted["del6"]] is True and st[self.planted["del5"]] is False
        self.eng = self.ix.engine()
        self.eng.indels_enable(32, 2, 10)


@pytest.fixture(scope="module")
def crafted():
    w = Crafted()
    yield w
    w.eng.close()
    w.ix.close()


class Hpv:
    """HPV16 at k = 21 with the indel tests' 2,000-read sample"""

    def __init__(self):
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.g = indels_ref.read_fasta(os.path.join(GOLDEN, "HPV16.fa"), K)
        self.reads, _ = indel_cases.sample_reads(self.g.text)
        self.res = indels_ref.indel_events(self.g, self.reads)
        self.events, self.sums = ref.events_of(self.res), self.res.span_sums()
        self.eng = self.ix.engine()
        self.eng.indels_enable()


@pytest.fixture(scope="module")
def hpv():
    w = Hpv()
    yield w
    w.eng.close()
    w.ix.close()


def _b(reads):
    return [r.encode() for r in reads]


def _to_call(eng, reads, indels=True):
    """A sample of the reads up to bk_sample_call, with the whole indel table reported"""
    eng.sample_begin()
    words, lens = pack_reads(_b(reads), K)
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    if indels:
        eng.sample_indels(1, 0)
    eng.sample_call(1)


TALLIES5 = ("positions", "called", "ambiguous", "masked", "substitutions")


def _step(eng, D, F):
    """bk_sample_consensus at (D, F) and the step behind it: (plain letters, summary, rows, edited letters)"""
    eng.sample_consensus(eng.consensus_params(min_depth=D, min_freq=F))
    before, plain = eng.download_consensus()
    eng.sample_consensus_indels()
    summ, rows = eng.download_consensus_indels()
    after, edited = eng.download_consensus()
    assert [getattr(before, n) for n in TALLIES5] == [getattr(after, n) for n in TALLIES5] and before.file_id == after.file_id   # those of the unedited letters
    return plain, summ, rows, edited


def _check(eng, w, D, F, what=""):
    plain, summ, rows, edited = _step(eng, D, F)
    assert summ.file_id == 0 and summ.overflow == 0 and len(plain) == w.g.cells and b"-" not in plain, what
    want_rows, want = ref.resolve(w.events, w.sums, D, F)
    assert rows == ref.abi_rows(want_rows), (what, D, F, [r for r in rows if r not in ref.abi_rows(want_rows)][:3], [r for r in ref.abi_rows(want_rows) if r not in rows][:3])
    assert {n: getattr(summ, n) for n in ref.TALLIES} == want, (what, D, F)
    want_letters = ref.edit_letters(plain, want_rows)
    if edited != want_letters:
        bad = [i for i in range(len(plain)) if edited[i:i + 1] != want_letters[i:i + 1]]
        raise AssertionError("%s at D = %d, F = %r: %d letters differ, first at %d" % (what, D, F, len(bad), bad[0]))
    return want, (summ, rows, edited)


def test_crafted_sample(crafted):
    _to_call(crafted.eng, crafted.reads)
    seen = {}
    for D, F in ref.PAIRS:
        seen[(D, F)], _ = _check(crafted.eng, crafted, D, F, "crafted")
    assert seen[(10, 0.5)]["deletions"] >= 1 and seen[(10, 0.5)]["insertions"] >= 1 and seen[(10, 0.25)]["contested"] >= 1
    assert seen[(1, 0.0)]["accepted"] == seen[(1, 0.0)]["candidates"] >= 5 and seen[(10, 0.5)]["frameshifts"] >= 1


@pytest.mark.parametrize("D,F", [(1, 0.0), (10, 0.5)])
def test_hpv16_sample(hpv, D, F):
    _to_call(hpv.eng, hpv.reads)
    want, _ = _check(hpv.eng, hpv, D, F, "hpv16")
    assert want["applied"] >= 1 and want["candidates"] >= 6


def test_second_grid_trip(crafted):
    """A table of 2^20 slots: the slot passes' grid of 2048 workgroups of 256 threads goes round twice.  The same result as at 2^10."""
    got = []
    for log2 in (10, 20):
        eng = crafted.ix.engine()
        try:
            eng.indels_enable(32, 2, log2)
            _to_call(eng, crafted.reads)
            got.append([_check(eng, crafted, D, F, log2)[1] for D, F in ((10, 0.25), (1, 0.0))])
        finally:
            eng.close()
    for x, y in zip(*got):
        assert x[1:] == y[1:] and [getattr(x[0], n) for n in ref.TALLIES] == [getattr(y[0], n) for n in ref.TALLIES]


def test_samples_in_a_row_and_a_fork(crafted):
    eng = crafted.eng
    plain_reads = [r for r in crafted.reads if not indels_ref.indel_events(crafted.g, [r]).events]
    empty = indels_ref.indel_events(crafted.g, plain_reads)
    assert not empty.events and len(plain_reads) > 100
    _to_call(eng, crafted.reads)
    first = _check(eng, crafted, 10, 0.5, "first")[0]
    assert first["applied"] >= 2
    _to_call(eng, plain_reads)                                       # the second sample has no indels: nothing of the first one shows
    plain, summ, rows, edited = _step(eng, 10, 0.5)
    assert rows == [] and edited == plain and b"-" not in edited and summ.file_id == 0 and summ.overflow == 0
    assert [getattr(summ, n) for n in ref.TALLIES] == [0] * 9
    _to_call(eng, crafted.reads)                                     # the step again behind a second bk_sample_consensus: that pair's result
    for D, F in ((10, 0.5), (10, 0.25), (10, 0.5), (1, 1.0)):
        _check(eng, crafted, D, F, "again")
    eng.sample_consensus_indels()                                    # ... and twice behind one: the same
    assert eng.download_consensus_indels()[1] == ref.abi_rows(ref.resolve(crafted.events, crafted.sums, 1, 1.0)[0])
    fork = eng.fork()
    try:
        fork.indels_enable(32, 2, 12)
        _to_call(fork, crafted.reads)
        a = _check(fork, crafted, 10, 0.25, "fork")[1]
        b = _check(eng, crafted, 10, 0.25, "parent")[1]
        assert a[1:] == b[1:]
    finally:
        fork.close()


def test_no_genome_selected(crafted):
    eng = crafted.ix.engine()
    try:
        eng.indels_enable(32, 2, 10)
        eng.sample_begin()
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        eng.sample_call(1)
        eng.sample_consensus()
        eng.sample_consensus_indels()
        summ, rows = eng.download_consensus_indels()
        assert summ.file_id == -1 and rows == [] and summ.overflow == 0 and [getattr(summ, n) for n in ref.TALLIES] == [0] * 9
    finally:
        eng.close()


def test_call_order(crafted):
    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    eng = crafted.ix.engine()
    try:
        st, msg = status(eng.sample_consensus_indels)                # indels not enabled
        assert st == -5 and "not enabled" in msg
        _to_call(eng, crafted.reads[:50], indels=False)
        eng.sample_consensus()
        st, msg = status(eng.sample_consensus_indels)
        assert st == -5 and "not enabled" in msg
        eng.indels_enable(32, 2, 10)
        st, msg = status(eng.sample_consensus_indels)                # enabled after the sample began
        assert st == -5 and "not enabled" in msg
        eng.sample_begin()
        st, msg = status(eng.sample_consensus_indels)                # inside a sample
        assert st == -5 and "comes after" in msg
        words, lens = pack_reads(_b(crafted.reads), K)
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        eng.sample_call(1)
        st, msg = status(eng.sample_consensus_indels)                # before bk_sample_consensus
        assert st == -5 and "bk_sample_consensus has not run" in msg
        assert status(eng.download_consensus_indels)[0] == -5
        _to_call(eng, crafted.reads, indels=False)
        eng.sample_consensus()
        st, msg = status(eng.sample_consensus_indels)                # before bk_sample_indels
        assert st == -5 and "bk_sample_indels has not run" in msg
        eng.sample_indels(5, 30000)                                  # its thresholds do not shape the candidates
        _check(eng, crafted, 10, 0.5, "order")
        eng.sample_consensus()                                       # fresh letters: the step is due again
        assert status(eng.download_consensus_indels)[0] == -5
        eng.sample_consensus_indels()
        summ, rows = eng.download_consensus_indels(cap=1)            # fewer than there are: `cap` rows, the full count
        assert len(rows) == 1 and summ.accepted > 1
        eng.sample_call(1)                                           # another selection: no letters, no result
        assert status(eng.sample_consensus_indels)[0] == -5 and status(eng.download_consensus_indels)[0] == -5
        eng.sample_begin()
        assert status(eng.download_consensus_indels)[0] == -5
    finally:
        eng.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(crafted, tmp_path):
    fasta = str(tmp_path / "crafted.fa")
    with open(fasta, "w") as f:
        for name, s in crafted.seqs:
            f.write(">%s\n%s\n" % (name, s))
    db = str(tmp_path / "crafted")
    res = subprocess.run([BRONKO, "build", "-g", fasta, "-k", str(K), "-t", "2", "-o", db], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    fq = str(tmp_path / "ci.fastq.gz")
    with gzip.open(fq, "wb", compresslevel=1) as f:
        for i, r in enumerate(_b(crafted.reads)):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    outs = {}
    for name, extra in (("with", ["--consensus-indels"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db + ".bkdb", "-r", fq, "--consensus", "--indels", "-o", out, "-t", "4"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("Consensus indels:" in res.stdout and "frameshifts" in res.stdout) == (name == "with"), res.stdout
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "ci"
    assert set(outs["with"]) == set(outs["without"]) | {stem + ".consensus_indels.tsv"}
    for f in outs["without"]:                                        # every other output does not know of the flag
        assert (outs["with"][f] == outs["without"][f]) == (f != stem + ".consensus.fa"), f
    _to_call(crafted.eng, crafted.reads)                             # the plain letters: the engine's own
    crafted.eng.sample_consensus()
    plain = crafted.eng.download_consensus()[1]
    path = str(tmp_path / "plain.fa")
    hostlib.write_consensus_fasta(path, stem, crafted.ix, 0, plain)
    assert outs["without"][stem + ".consensus.fa"] == open(path, "rb").read()   # without the flag: the consensus of today
    rows, t = ref.resolve(crafted.events, crafted.sums, 10, 0.5)
    edited = ref.edit_letters(plain, rows)
    assert t["deletions"] >= 1 and t["insertions"] >= 1
    assert outs["with"][stem + ".consensus.fa"].decode() == ref.fasta_text(crafted.g, stem, edited, rows)
    assert outs["with"][stem + ".consensus_indels.tsv"].decode() == ref.tsv_text(crafted.g, edited, rows, 10, 0.5)
