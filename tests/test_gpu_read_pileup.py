"""bk_sample_read_pileup / bk_sample_download_read_pileup (bk_read_pileup.hip) against the Python restatement of the rule
(tests/read_pileup_ref.py) and the host twin (read_pileup.cpp): the twelve counters of every cell and the summary must be equal --
the rule is integer arithmetic, no case is left out.  Then the call order of the C ABI, what the feature must leave alone, and
`bronko call --read-pileup` end to end."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, hostlib, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import codon_cases, haplotype_cases, indel_cases, indels_ref, linkage_ref, read_pileup_ref
from tests.linkage_cases import N_LEN, START

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _sample(eng, reads, k=K):
    eng.sample_begin()
    if reads:
        _packed(eng, 0, reads, k)
    eng.sample_finalize(1)


def _check(eng, ix, g, rows, E, what=""):
    """The finalized sample's read pileup at end distance E against the restatement of `rows` and against the twin of the engine's rows"""
    eng.sample_read_pileup(E)
    summ, cells = eng.download_read_pileup()
    want = read_pileup_ref.read_pileup(g, rows, E)
    assert cells.shape == want.shape and np.array_equal(cells, want), (what, E, np.argwhere(cells != want)[:5].tolist())
    covered, bases = read_pileup_ref.summary(want, rows)
    assert (summ.rows, summ.n_cells, summ.end_dist, summ.covered, summ.bases) == (len(rows), g.cells, E, covered, bases), (what, E)
    twin = hostlib.read_pileup_count(ix, 0, eng.download_link_rows(raw=True), E)
    assert np.array_equal(twin, want), (what, E, "twin")
    return want


def _one(eng, ix, g, reads, M, ends, k=K, what=""):
    rows, t = linkage_ref.link_rows(g, reads, M)
    _sample(eng, reads, k)
    return rows, [_check(eng, ix, g, rows, E, what) for E in ends]


class World:
    """haplotype_cases' planted sample (HPV16, k = 21) with the index and an engine that has linkage enabled"""

    def __init__(self):
        self.p = haplotype_cases.planted()
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.eng = self.ix.engine()
        self.eng.linkage_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


class Crafted:
    def __init__(self, k):
        self.k = k
        self.seqs = indel_cases.crafted_genome(k)
        self.ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in self.seqs])])
        self.g = indels_ref.Genome([name.split()[0] for name, _ in self.seqs], [s for _, s in self.seqs], k)
        self.eng = self.ix.engine()
        self.eng.linkage_enable(8, 16)


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    c = Crafted(request.param)
    yield c
    c.eng.close()
    c.ix.close()


def test_crafted_records_on_both_strands_and_both_sequences(crafted):
    c = crafted
    reads = [r for _, r in haplotype_cases.crafted_cases(c.k)]
    for M in (0, 2, 8):
        c.eng.linkage_enable(M, 16)
        rows, (at10, at0, at255) = _one(c.eng, c.ix, c.g, reads, M, (10, 0, 255), c.k, what=(c.k, M))
        assert {r[2] for r in rows} == {0, 1} and c.g.seq_of(max(r[0] for r in rows)) == 1
        assert at0[:, 8:].sum() == 0 and np.array_equal(at255[:, 8:], at255[:, :4] + at255[:, 4:8])   # E = 0: no cell; E above every length: every cell
        assert (at10[1300:1320] == 0).all() and at10[START, :8].sum() >= 2                             # nothing over the stretch of N
        assert max(len(r[3]) for r in rows) == M
    c.eng.linkage_enable(8, 16)


def test_eight_substitutions_of_which_some_are_near_an_end(crafted):
    c = crafted
    by = dict(haplotype_cases.crafted_cases(c.k))
    for E in (41, 47, 10):                                         # mm_8: offsets 40, 49, .. 103 of 150: one near an end from 41 on, two from 47 on
        rows, (got,) = _one(c.eng, c.ix, c.g, [by["mm_8"], by["mm_8/rc"]], 8, (E,), c.k, what="mm_8")
        assert [len(r[3]) for r in rows] == [8, 8] and sorted(r[2] for r in rows) == [0, 1]
        near_subs = sum(int(got[START + o, 8:].sum()) for o in range(40, 104, 9))
        assert near_subs == {41: 2, 47: 4, 10: 0}[E] and sum(int(got[START + o, :8].sum()) for o in range(40, 104, 9)) == 16


def test_rows_of_length_two_e_one_less_and_one_more(crafted):
    c = crafted
    a, E = c.seqs[0][1], c.k + 3
    reads = [indel_cases.mut_read(a, START + 7 * i, n, subs=tuple(sorted({E - 1, E, n - E - 1})) if n > 2 * E else (c.k + 1, c.k + 3))
             for i, n in enumerate((2 * E - 1, 2 * E, 2 * E + 1, 2 * E + 2))]
    reads += [indels_ref.revcomp(r) for r in reads]
    rows, _ = _one(c.eng, c.ix, c.g, reads, 8, (E, E - 1, E + 1, 0, 255), c.k, what="2E")
    assert sorted(r[1] for r in rows) == sorted([2 * E - 1, 2 * E, 2 * E + 1, 2 * E + 2] * 2)


def test_rows_at_the_first_and_the_last_cell_of_each_sequence(crafted):
    """The row that ends at the last cell of the last sequence adds its -1 to word total_cells of the difference arrays."""
    c = crafted
    a, b, k = c.seqs[0][1], c.seqs[1][1], c.k
    reads = [a[:N_LEN], indels_ref.revcomp(a[len(a) - N_LEN:]), b[:N_LEN], b[len(b) - N_LEN:], indels_ref.revcomp(b[len(b) - 2 * k:])]
    rows, (got, _, _) = _one(c.eng, c.ix, c.g, reads, 8, (10, k, 255), k, what="borders")
    assert {(r[0], r[0] + r[1]) for r in rows} >= {(0, N_LEN), (len(a) - N_LEN, len(a)), (len(a), len(a) + N_LEN), (c.g.cells - N_LEN, c.g.cells), (c.g.cells - 2 * k, c.g.cells)}
    assert got[c.g.cells - 1, :8].sum() == 2 and got[0, :4].sum() == 1 and got[len(a) - 1, 4:8].sum() == 1 and got[len(a), :4].sum() == 1


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    p = world.p
    placed = [r for r in p.reads if linkage_ref.place(p.g, linkage_ref.records_of(r, K)[0], 8)[0] == "placed"]
    rows, _ = _one(world.eng, world.ix, p.g, placed[:n], 8, (10,), what=n)
    assert len(rows) == n


def test_two_thousand_rows_from_one_cell_with_shared_substitutions(world):
    """Every lane of every wave adds to the same few words: the merged adds are exact."""
    p = world.p
    reads = haplotype_cases.hot_reads(p.g.text)
    rows, (got, _) = _one(world.eng, world.ix, p.g, reads, 8, (12, 0), what="hot")
    assert len(rows) == 2000 and len({r[0] for r in rows}) == 1
    at = haplotype_cases.HOT_START
    assert got[at, :4].sum() == 1000 and got[at, 4:8].sum() == 1000 and got[at + 10, 8:].max() == 2000 and got[at + 12, 8:].sum() == 0
    assert sorted(got[at + 73, :8].tolist()) == [0] * 6 + [1000, 1000]


def test_amplicon_reads_of_two_haplotypes_with_errors(world):
    p = world.p
    noisy = codon_cases.sample_reads(p.g.text, seed=7, n_reads=2000, span=(1990, 1990 + 151))
    rows, (got,) = _one(world.eng, world.ix, p.g, noisy, 8, (10,), what="one amplicon")
    assert len(rows) > 1800 and len({r[0] for r in rows}) <= 2 and got[:, :8].sum(axis=1).max() == len(rows)


def test_two_counts_with_another_e_and_a_second_sample_from_zero(world):
    p, eng = world.p, world.eng
    _sample(eng, p.reads)
    a = _check(eng, world.ix, p.g, p.rows, 10, "first")
    b = _check(eng, world.ix, p.g, p.rows, 30, "second")
    assert not np.array_equal(a[:, 8:], b[:, 8:]) and np.array_equal(a[:, :8], b[:, :8])
    _check(eng, world.ix, p.g, p.rows, 10, "the first again")
    summ, cells = eng.download_read_pileup(cap=7)                  # fewer than there are: `cap` cells from cell 0 on, the full summary
    assert cells.shape == (7, 12) and summ.n_cells == p.g.cells and summ.bases == sum(r[1] for r in p.rows)
    few = p.reads[:50]
    rows, (got,) = _one(eng, world.ix, p.g, few, 8, (10,), what="a second sample")   # nothing of the first sample is left
    assert got[:, :8].sum() == sum(r[1] for r in rows) < a[:, :8].sum()
    _sample(eng, [])
    _check(eng, world.ix, p.g, [], 10, "an empty sample")


def test_call_order_and_parameters(world):
    p = world.p
    eng = world.ix.engine()

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        assert status(eng.sample_read_pileup)[0] == -5               # linkage is not enabled
        assert status(eng.download_read_pileup)[0] == -5
        eng.linkage_enable()
        assert status(eng.sample_read_pileup)[0] == -5               # nothing was ever begun
        eng.sample_begin()
        assert status(eng.sample_read_pileup)[0] == -5               # inside a sample
        _packed(eng, 0, p.reads[:300])
        eng.sample_finalize(1)
        assert status(eng.download_read_pileup)[0] == -5             # before the count of this sample
        st, msg = status(eng.sample_read_pileup, 256)
        assert st == -1 and "256" in msg, msg
        assert status(eng.download_read_pileup)[0] == -5             # a refused call counted nothing
        rows, _ = linkage_ref.link_rows(p.g, p.reads[:300], 8)
        want = _check(eng, world.ix, p.g, rows, 10)                  # needs the finalize only, not bk_sample_call
        eng.sample_call(1)
        _check(eng, world.ix, p.g, rows, 255)
        assert status(eng.sample_read_pileup, 256)[0] == -1
        assert np.array_equal(eng.download_read_pileup()[1][:, :8], want[:, :8])   # a refused call leaves the last result alone
        assert eng._L.bk_sample_download_read_pileup(eng.h, None, None, 0) == -1
        eng.sample_begin()                                           # the next sample: nothing is this sample's yet
        assert status(eng.download_read_pileup)[0] == -5 and status(eng.sample_read_pileup)[0] == -5
        eng.sample_finalize(1)
        assert status(eng.download_read_pileup)[0] == -5
        _check(eng, world.ix, p.g, [], 10, "an empty sample")
        eng.linkage_enable(None)                                     # the buffers go with the row store
        assert status(eng.download_read_pileup)[0] == -5
    finally:
        eng.close()


def test_every_other_result_is_the_same_with_a_read_pileup_count_in_between(world):
    p = world.p
    plain, used = world.ix.engine(), world.ix.engine()
    sites = [codon_cases.SAMPLE_P + o for o in (0, 2, 30, 63)]
    try:
        out = []
        for eng in (plain, used):
            eng.linkage_enable(8, 4096)
            eng.sample_begin()
            _packed(eng, 0, p.reads[:1000])
            _packed(eng, 1, p.reads[1000:])
            res = eng.sample_finish(2)
            eng.sample_linkage(sites, 1000)
            if eng is used:
                _check(eng, world.ix, p.g, p.rows, 10)
            eng.sample_codons(p.frames[:1])
            eng.sample_haplotypes(p.regs_a, 12)
            if eng is used:
                _check(eng, world.ix, p.g, p.rows, 3)
            eng.sample_call(2)
            summ, recs = eng.download_calls()
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        eng.download_linkage()[1], eng.download_link_rows(), eng.download_codons()[1].tobytes(),
                        [list(x) if i < 2 else x for i, x in enumerate(eng.download_haplotypes()[1:])]))
        for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
            assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
        assert out[0][1:] == out[1][1:] and out[0][1][1] > 0 and len(out[0][3]) == 6
        assert out[1][6][2] == p.table_a[2] and out[1][4] == p.rows
    finally:
        plain.close()
        used.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_cli_read_pileup_end_to_end(world, tmp_path):
    p = world.p
    reads = _b(p.reads)
    path = str(tmp_path / "rp_R1.fastq.gz")
    with gzip.open(path, "wb", compresslevel=1) as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    genes = str(tmp_path / "genes.bed")
    with open(genes, "w") as f:
        for c0, nc, _, start, strand, name in p.genes:
            f.write("HPV16REF\t%d\t%d\t%s\t0\t%s\n" % (start, start + 3 * nc, "" if name == "." else name, strand))
    lines = open(os.path.join(GOLDEN, "HPV16.fa")).read().split("\n")
    names, letters = [lines[0][1:].split()[0]], ["".join(lines[1:])]
    assert letters[0].upper() == p.g.text
    db = os.path.join(GOLDEN, "hpv.bkdb")
    others = ["--linkage", "--codons", genes, "--hap-window", "100", "--hap-step", "50"]
    outs, logs = {}, {}
    # the flag alone turns the row store on, with its own M; beside the other three readers of the store it takes the defaults
    for name, extra in (("alone", ["--read-pileup", "--read-pileup-end", "0", "--read-pileup-max-mismatches", "2"]), ("all", ["--read-pileup"] + others), ("others", others),
                        ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db, "-r", path, "--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("Read pileup:" in res.stdout) == ("--read-pileup" in extra)
        outs[name], logs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}, res.stdout
    stem = "rp_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    seen = set()
    for name, (M, E) in (("alone", (2, 0)), ("all", (8, 10))):
        base = "others" if name == "all" else "without"
        assert set(outs[name]) == set(outs[base]) | {stem + ".read_pileup.tsv"}
        for f in outs[base]:                                       # every other output does not know of the flag
            assert outs[name][f] == outs[base][f], (name, f)
        rows = p.rows if M == 8 else linkage_ref.link_rows(p.g, p.reads, M)[0]
        counts = read_pileup_ref.read_pileup(p.g, rows, E)
        want = read_pileup_ref.tsv_text(names, letters, counts, M, E)
        assert outs[name][stem + ".read_pileup.tsv"].decode() == want, name
        covered, bases = read_pileup_ref.summary(counts, rows)
        assert "Read pileup: %d placed records, %d of %d positions covered, %d bases" % (len(rows), covered, p.g.cells, bases) in logs[name], logs[name]
        seen.add(want)
    assert len(seen) == 2
    # the first eleven columns are --pileup's: the same header, the same reference columns on every line
    head = lambda text: [ln.split("\t")[:3] for ln in text.splitlines() if not ln.startswith("##")]
    assert [h[:3] for h in head(outs["all"][stem + ".read_pileup.tsv"].decode())] == head(outs["all"][stem + ".tsv"].decode())
