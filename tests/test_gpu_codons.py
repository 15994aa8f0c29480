"""bk_sample_codons / bk_sample_download_codons (bk_codons.hip) against the Python restatement of the rule (tests/codons_ref.py): every
counter of every codon and the summary must be equal -- the rule is integer arithmetic, no case is left out.  Then both paths of the
cover difference array, the call order of the C ABI, what the feature must leave alone, and `bronko call --codons` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads
from bronko_amd.engine import device_memory
from bronko_amd.hostlib import HostIndex
from tests import codon_cases, codons_ref, indel_cases, indels_ref, linkage_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21
LDS_CODONS = 16384                   # kCodonLdsCodons: a cover difference array of more entries takes the global path


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _sample(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    eng.sample_finalize(1)


def _check(eng, n_rows, regions, want, what=""):
    """The finalized sample's counter table and summary for `regions` against `want`"""
    eng.sample_codons(regions)
    summ, got = eng.download_codons()
    assert (summ.rows, summ.n_codons, summ.n_regions) == (n_rows, len(want), len(regions)), what
    assert got.shape == want.shape and np.array_equal(got, want), (what, [(int(i), got[i].nonzero(), want[i].nonzero()) for i in np.flatnonzero((got != want).any(axis=1))[:3]])
    return got


def _one(eng, g, reads, M, regions, k=K, what=""):
    rows, t = linkage_ref.link_rows(g, reads, M)
    _sample(eng, reads, k)
    return _check(eng, t["placed"], regions, codons_ref.codon_count(g, rows, regions), what)


class World(codon_cases.Planted):
    """... with the index and an engine that has linkage enabled"""

    def __init__(self):
        super().__init__(K)
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.eng = self.ix.engine()
        self.eng.linkage_enable()
        self.regs = codons_ref.regions_of(self.genes)
        self.placed = self.tallies["placed"]
        assert len(self.counts) + 1 <= LDS_CODONS < 3 * len(self.counts) + 1


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


def _other(g, regions, counts):
    """the counts that are not the reference triplet's"""
    total, c = 0, 0
    for c0, nc in regions:
        for i in range(nc):
            ref = g.text[c0 + 3 * i:c0 + 3 * i + 3]
            if "N" not in ref:
                total += int(counts[c].sum()) - int(counts[c, sum("ACGT".index(x) << (4 - 2 * j) for j, x in enumerate(ref))])
            c += 1
    return total


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records(k):
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r in codon_cases.crafted_cases(k)]
    regions = codon_cases.crafted_regions(k)
    eng = ix.engine()
    try:
        for M in (0, 2, 8):
            eng.linkage_enable(M, 16)
            got = _one(eng, g, reads, M, regions, k, what=(k, M))
            other = _other(g, regions, got)
            assert (other == 0) if M == 0 else (other > 50 if M == 8 else other > 10), (M, other)
        rows, t = linkage_ref.link_rows(g, reads, 8)                # the same sample, the regions in another order
        _check(eng, t["placed"], regions[::-1], codons_ref.codon_count(g, rows, regions[::-1]), "reversed")
    finally:
        eng.close()
        ix.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    placed = [r for r in world.reads if linkage_ref.place(world.g, linkage_ref.records_of(r, K)[0], 8)[0] == "placed"]
    got = _one(world.eng, world.g, placed[:n], 8, world.frames, what=n)
    assert int(got.sum()) > 140 * n


def test_the_sample_whole_and_in_pieces_over_two_mate_files(world):
    eng = world.eng
    for cuts in ([0, 2000], [0, 37, 700, 1301, 2000]):
        eng.sample_begin()
        for a, b in zip(cuts, cuts[1:]):
            _packed(eng, 0 if b <= 1000 or len(cuts) == 2 else 1, world.reads[a:b])
        eng.sample_finalize(1 if len(cuts) == 2 else 2)
        _check(eng, world.placed, world.frames, world.counts, what=len(cuts))
        _check(eng, world.placed, world.regs, world.gene_counts, what=("genes", len(cuts)))


def test_lds_path_global_path_and_both_agree(world):
    eng = world.eng
    _sample(eng, world.reads)
    small = _check(eng, world.placed, world.frames, world.counts, what="three frames")          # 7.9 k codons: privatised in LDS
    large = _check(eng, world.placed, world.frames * 3, np.concatenate([world.counts] * 3), what="nine regions")   # 23.7 k: global atomics
    assert len(small) + 1 <= LDS_CODONS < len(large) + 1
    assert np.array_equal(large[:len(small)], small) and np.array_equal(large[2 * len(small):], small)   # the shared regions under both paths
    assert _other(world.g, world.frames, small) > 1000 and int(small.sum()) > 140 * world.placed
    for extra, path in ((LDS_CODONS - 1 - 2 * len(small), "the largest in LDS"), (LDS_CODONS - 2 * len(small), "the smallest in device memory")):
        regions = world.frames * 2 + [(0, extra)]                                               # 16,383 and 16,384 codons
        _check(eng, world.placed, regions, np.concatenate([small, small, small[:extra]]), what=path)


def test_two_thousand_reads_that_start_at_one_cell(world):
    """Amplicon reads: every row adds to the same two entries of the difference array and, for the planted substitutions, to the
    same counters."""
    hap = codon_cases.sample_reads(world.g.text, seed=7, n_reads=2000, span=(1990, 1990 + 151))
    rows, t = linkage_ref.link_rows(world.g, hap, 8)
    assert t["placed"] > 1800 and len({r[0] for r in rows}) == 1
    _sample(world.eng, hap)
    want = codons_ref.codon_count(world.g, rows, world.frames)
    got = _check(world.eng, t["placed"], world.frames, want, what="one start")
    assert int(got.max()) > 1800
    _check(world.eng, t["placed"], world.frames * 3, np.concatenate([want] * 3), what="one start, global path")


def test_again_with_other_regions_no_regions_and_a_small_cap(world):
    eng = world.eng
    _sample(eng, world.reads)
    _check(eng, world.placed, world.frames, world.counts)
    _check(eng, world.placed, world.regs, world.gene_counts)                          # fewer codons: the old counters are zeroed, not added to
    _check(eng, world.placed, world.regs[:1], world.gene_counts[:100])
    _check(eng, world.placed, [], np.zeros((0, 64), np.uint32), what="no regions")
    summ, got = eng.download_codons(cap=3)
    assert len(got) == 0 and (summ.n_codons, summ.n_regions) == (0, 0)
    _check(eng, world.placed, world.regs, world.gene_counts)
    summ, got = eng.download_codons(cap=7)                                            # fewer than there are: `cap` rows, the full count
    assert summ.n_codons == len(world.gene_counts) and np.array_equal(got, world.gene_counts[:7])
    raw, s2 = np.full((12, 64), 0xffffffff, np.uint32), _ffi.CodonSummary()
    assert eng._L.bk_sample_download_codons(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 5) == 0
    assert np.array_equal(raw[:5], world.gene_counts[:5]) and (raw[5:] == 0xffffffff).all()   # the rows beyond cap are untouched
    assert eng._L.bk_sample_download_codons(eng.h, None, raw.ctypes.data_as(C.c_void_p), 2) == 0
    assert eng._L.bk_sample_download_codons(eng.h, None, None, 0) == -1


@pytest.mark.parametrize("order", ["linkage_first", "codons_first"])
def test_linkage_and_codons_on_one_sample(world, order):
    eng = world.eng
    sites = [codon_cases.SAMPLE_P + o for o in (0, 2, 30, 63, 64, 65, 100)]
    pairs = linkage_ref.link_count(world.g, world.rows, sites, 1000)
    _sample(eng, world.reads)
    if order == "linkage_first":
        eng.sample_linkage(sites, 1000)
        eng.sample_codons(world.regs)
    else:
        eng.sample_codons(world.regs)
        eng.sample_linkage(sites, 1000)
    summ, got = eng.download_linkage()
    assert got == pairs and summ.placed == world.placed
    summ, counts = eng.download_codons()
    assert np.array_equal(counts, world.gene_counts) and summ.rows == world.placed
    eng.sample_codons(world.frames)                                                   # ... and again: linkage's counters stay
    assert np.array_equal(eng.download_codons()[1], world.counts) and eng.download_linkage()[1] == pairs


def test_an_engine_its_fork_and_a_store_that_grew(world):
    fork = world.eng.fork()
    try:
        _sample(fork, world.reads[:100])                            # a fork has no row store of its parent's
        with pytest.raises(BronkoError) as ei:
            fork.sample_codons(world.regs)
        assert ei.value.status == -5
        fork.linkage_enable(8, 64)                                  # 64 rows, 2,000 records, four pushes
        fork.sample_begin()
        for a, b in ((0, 37), (37, 700), (700, 1301), (1301, 2000)):
            _packed(fork, 0, world.reads[a:b])
        fork.sample_finalize(1)
        _check(fork, world.placed, world.frames, world.counts, what="grown store")
        for e, n in ((world.eng, 2000), (fork, 500), (world.eng, 1000)):
            _one(e, world.g, world.reads[:n], 8, world.regs, what=n)
    finally:
        fork.close()


def test_call_order_and_parameters(world):
    eng = world.ix.engine()

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        assert status(eng.sample_codons, world.regs)[0] == -5         # linkage is not enabled
        eng.linkage_enable()
        assert status(eng.sample_codons, world.regs)[0] == -5         # nothing was ever begun
        assert status(eng.download_codons)[0] == -5
        eng.sample_begin()
        assert status(eng.sample_codons, world.regs)[0] == -5         # inside a sample
        _packed(eng, 0, world.reads[:300])
        assert status(eng.sample_codons, world.regs)[0] == -5         # before the finalize
        eng.sample_finalize(1)
        rows, t = linkage_ref.link_rows(world.g, world.reads[:300], 8)
        summ, got = eng.download_codons()                             # before the first count: the rows and no codons
        assert (summ.rows, summ.n_codons, summ.n_regions, len(got)) == (t["placed"], 0, 0, 0)
        cells = world.g.cells
        for bad, word in (([(5, 3), (9, 0)], "region 1"), ([(0, 1), (5, 2), (cells - 5, 2)], "region 2"), ([(cells, 1)], "region 0"),
                          ([(0, 1)] * 4097, "4097"), ([(0, 2600)] * 101, "262600")):
            st, msg = status(eng.sample_codons, bad)
            assert st == -1 and word in msg, (bad[:3], msg)
        summ, got = eng.download_codons()                             # no launch was made, nothing was counted
        assert (summ.rows, summ.n_codons, len(got)) == (t["placed"], 0, 0)
        want = codons_ref.codon_count(world.g, rows, world.regs)
        _check(eng, t["placed"], world.regs, want)                    # needs the finalize only, not bk_sample_call
        eng.sample_call(1)
        _check(eng, t["placed"], world.regs, want)                    # ... and after the call as well
        assert status(eng.sample_codons, [(5, 0)])[0] == -1
        assert np.array_equal(eng.download_codons()[1], want)         # a refused call leaves the last table alone
        eng.sample_begin()                                            # the next sample: nothing is this sample's yet
        assert status(eng.download_codons)[0] == -5 and status(eng.sample_codons, world.regs)[0] == -5
        eng.sample_finalize(1)
        summ, got = eng.download_codons()
        assert (summ.rows, summ.n_codons, len(got)) == (0, 0, 0)
        _check(eng, 0, world.regs, np.zeros_like(want), what="an empty sample")
        eng.linkage_enable(None)                                      # the counters go with the row store
        assert status(eng.download_codons)[0] == -5
    finally:
        eng.close()
    seqs = indel_cases.crafted_genome(K)                              # two sequences: a region across their border
    ix2 = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in seqs])])
    eng2 = ix2.engine()
    try:
        eng2.linkage_enable()
        _sample(eng2, [seqs[0][1][900:1050]])
        n_a = len(seqs[0][1])
        st, msg = status(eng2.sample_codons, [(n_a - 30, 10), (n_a - 3, 2)])
        assert st == -1 and "region 1" in msg and "border" in msg, msg
        eng2.sample_codons([(n_a - 30, 10), (n_a, 2)])
    finally:
        eng2.close()
        ix2.close()


def test_every_other_result_is_the_same_and_nothing_is_allocated_without_the_call(world):
    plain, used = world.ix.engine(), world.ix.engine()
    sites = [codon_cases.SAMPLE_P + o for o in (0, 2, 30, 63)]
    try:
        out = []
        for eng in (plain, used):
            eng.linkage_enable(8, 4096)
            free = []
            for rep in range(3):
                eng.sample_begin()
                _packed(eng, 0, world.reads[:1000])
                _packed(eng, 1, world.reads[1000:])
                res = eng.sample_finish(2)
                if eng is used:
                    eng.sample_codons(world.frames)
                    assert np.array_equal(eng.download_codons()[1], world.counts)
                eng.sample_call(2)
                summ, recs = eng.download_calls()
                eng.sample_linkage(sites, 1000)
                free.append(device_memory(0)[0])
            # an engine that never counts codons allocates nothing after its first sample; one that does, nothing after its first count
            assert free[1] == free[0] and free[2] == free[0], (eng is used, free)
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        eng.download_linkage()[1], eng.download_link_rows()))
        for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
            assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
        assert out[0][1:] == out[1][1:] and out[0][1][1] > 0 and len(out[0][3]) == 6    # (the same calls, pairs and rows; the sample has calls)
    finally:
        plain.close()
        used.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_codons_end_to_end(world, tmp_path, paired):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("cdn_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    bed = str(tmp_path / "genes.bed")
    with open(bed, "w") as f:
        f.write("# chrom\tstart\tend\tname\tscore\tstrand\n")
        for c0, nc, _, start, strand, name in world.genes:
            f.write("HPV16REF\t%d\t%d\t%s\t0\t%s\n" % (start, start + 3 * nc, "" if name == "." else name, strand))
    assert codons_ref.read_bed(world.g, bed) == world.genes
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("codons", ["--codons", bed]), ("strict", ["--codons", bed, "--codon-max-mismatches", "3", "--codon-min-reads", "50", "--codon-min-freq", "0.5"]),
                        ("both", ["--codons", bed, "--linkage"]), ("linkage", ["--linkage"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra,
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("codons counted" in res.stdout) == ("--codons" in extra)
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "cdn_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    seen = set()
    for name, (M, N, F) in (("codons", (8, 5, 0.03)), ("strict", (3, 50, 0.5)), ("both", (8, 5, 0.03))):
        base = "linkage" if name == "both" else "without"
        assert set(outs[name]) == set(outs[base]) | {stem + ".codons.tsv"}
        for f in outs[base]:                                       # every other output does not know of the flag
            assert outs[name][f] == outs[base][f], (name, f)
        rows, _ = linkage_ref.link_rows(world.g, world.reads, M)
        want = codons_ref.tsv_text(world.g, world.genes, codons_ref.codon_count(world.g, rows, world.regs), M, N, F)
        assert want.count("\n") >= 5                                # four header lines and at least one triplet
        assert outs[name][stem + ".codons.tsv"].decode() == want, name
        seen.add(want)
    assert len(seen) == 2
