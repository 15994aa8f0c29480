"""bk_sample_haplotypes / bk_sample_download_haplotypes (bk_haplotypes.hip) against the Python restatement of the rule
(tests/haplotypes_ref.py): cover, ref_count, every entry and the summary must be equal -- the rule is integer arithmetic, no case is
left out.  Then the table when it is tight and when it is full, the region index at its largest, the call order of the C ABI, what the
feature must leave alone, and `bronko call --haplotypes` / `--hap-window` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads
from bronko_amd.engine import device_memory
from bronko_amd.hostlib import HostIndex
from tests import codon_cases, codons_ref, haplotype_cases, haplotypes_ref, indel_cases, indels_ref, linkage_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21
MAX_REGIONS = 4096                   # BK_HAP_MAX_REGIONS: region index 4,095 is the largest that is packed into an owner word


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _sample(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    eng.sample_finalize(1)


def _check(eng, n_rows, regions, want, log2=16, what=""):
    """The finalized sample's haplotype table and summary for `regions` against `want` = (cover, ref_count, entries)"""
    eng.sample_haplotypes(regions, log2)
    summ, cover, ref, entries = eng.download_haplotypes()
    assert (summ.rows, summ.n_regions, summ.table_log2, summ.dropped, summ.entries) == (n_rows, len(regions), log2, 0, len(want[2])), what
    assert (list(cover), list(ref)) == (list(want[0]), list(want[1])), (what, [(i, a, b) for i, (a, b) in enumerate(zip(zip(cover, ref), zip(want[0], want[1]))) if a != b][:3])
    assert entries == want[2], (what, [x for x in zip(entries, want[2]) if x[0] != x[1]][:3])
    return cover, ref, entries


def _one(eng, g, reads, M, regions, k=K, log2=16, what=""):
    rows, t = linkage_ref.link_rows(g, reads, M)
    _sample(eng, reads, k)
    return _check(eng, t["placed"], regions, haplotypes_ref.hap_count(g, rows, regions), log2, what)


class World:
    """haplotype_cases' planted sample with the index and an engine that has linkage enabled"""

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


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records(k):
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r in haplotype_cases.crafted_cases(k)]
    regions = haplotype_cases.crafted_regions(k)
    eng = ix.engine()
    try:
        for M in (0, 2, 8):
            eng.linkage_enable(M, 16)
            cover, ref, entries = _one(eng, g, reads, M, regions, k, what=(k, M))
            assert (len(entries) == 0) if M == 0 else (len(entries) > 30 if M == 8 else len(entries) > 10), (M, len(entries))
            assert cover[regions.index((1290, 40))] == 0 and cover[0] >= 2   # (plain and plain/rc at every M)
        rows, t = linkage_ref.link_rows(g, reads, 8)                # the same sample, the regions in another order
        _check(eng, t["placed"], regions[::-1], haplotypes_ref.hap_count(g, rows, regions[::-1]), what="reversed")
    finally:
        eng.close()
        ix.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    p = world.p
    placed = [r for r in p.reads if linkage_ref.place(p.g, linkage_ref.records_of(r, K)[0], 8)[0] == "placed"]
    cover, _, _ = _one(world.eng, p.g, placed[:n], 8, p.regs_a, what=n)
    assert sum(cover) >= n


def test_two_thousand_reads_of_one_haplotype_from_one_cell(world):
    """Every lane of every wave claims the same empty slot at once and then adds to the same counter: the count is exact."""
    p = world.p
    reads = haplotype_cases.hot_reads(p.g.text)
    rows, t = linkage_ref.link_rows(p.g, reads, 8)
    assert t["placed"] == 2000 and len({r[0] for r in rows}) == 1
    _sample(world.eng, reads)
    want = haplotypes_ref.hap_count(p.g, rows, haplotype_cases.HOT_REGIONS)
    cover, ref, entries = _check(world.eng, 2000, haplotype_cases.HOT_REGIONS, want, what="one haplotype")
    assert [(r, n, len(h)) for r, n, h in entries] == [(0, 2000, 3), (1, 2000, 2), (3, 2000, 1), (4, 2000, 2)] and list(ref) == [0, 0, 2000, 0, 0]
    _check(world.eng, 2000, haplotype_cases.HOT_REGIONS, want, log2=10, what="one haplotype, the smallest table")
    noisy = codon_cases.sample_reads(p.g.text, seed=7, n_reads=2000, span=(1990, 1990 + 151))   # amplicon reads of two haplotypes with errors
    cover, ref, entries = _one(world.eng, p.g, noisy, 8, haplotype_cases.HOT_REGIONS + p.regs_a, what="one start")
    assert cover[0] > 1800 and max(n for _, n, _ in entries) > 500


def test_a_tight_table_a_full_table_and_the_same_sample_again(world):
    p, eng = world.p, world.eng
    _sample(eng, p.reads)
    _check(eng, p.placed, p.regs_a, p.table_a, log2=10, what="752 haplotypes in 1,024 slots")
    eng.sample_haplotypes(p.regs_b, 10)                                                # 2,948 haplotypes: the table is full
    with pytest.raises(BronkoError) as ei:
        eng.download_haplotypes()
    summ, cover, ref = ei.value.hap
    assert ei.value.status == -6 and "table_log2 = 10" in str(ei.value) and str(int(summ.dropped)) in str(ei.value), str(ei.value)
    assert summ.dropped > 0 and (summ.rows, summ.n_regions, summ.table_log2) == (p.placed, len(p.regs_b), 10)
    assert (list(cover), list(ref)) == (p.table_b[0], p.table_b[1])                    # the hot counters are exact all the same
    assert summ.dropped <= sum(c - r for c, r in zip(cover, ref)) and summ.entries <= 1024
    raw, s2 = np.full((4, 40), 0xff, np.uint8), _ffi.HapSummary()
    assert eng._L.bk_sample_download_haplotypes(eng.h, C.byref(s2), None, None, raw.ctypes.data_as(C.c_void_p), 4) == -6 and (raw == 0xff).all()   # no entry is copied
    _check(eng, p.placed, p.regs_b, p.table_b, log2=12, what="the same rows, a table of 4,096 slots")
    _check(eng, p.placed, p.regs_a, p.table_a, log2=11, what="a smaller table again")


def test_four_thousand_and_ninety_six_regions(world):
    p, eng = world.p, world.eng
    last = codon_cases.SAMPLE_P + 1500                                                 # a planted substitution: the last region has a haplotype of its own
    regions = [(last - (MAX_REGIONS - 1 - i) // 2, 1) for i in range(MAX_REGIONS)]     # every cell twice: 32 KiB of hot counters, region index 4,095
    _sample(eng, p.reads)
    cover, ref, entries = _check(eng, p.placed, regions, haplotypes_ref.hap_count(p.g, p.rows, regions), what="4,096 regions")
    assert entries[-1][0] == MAX_REGIONS - 1 and entries[-1][1] > 20 and entries[-2][:2] == (MAX_REGIONS - 2, entries[-1][1]) and cover[-1] > 50
    with pytest.raises(BronkoError) as ei:
        eng.sample_haplotypes(regions + [(5, 1)])
    assert ei.value.status == -1 and "4097" in str(ei.value)
    assert eng.download_haplotypes()[3] == entries                                     # a refused call leaves the last table alone


def test_the_sample_whole_and_in_pieces_over_two_mate_files(world):
    p, eng = world.p, world.eng
    for cuts in ([0, 2000], [0, 37, 700, 1301, 2000]):
        eng.sample_begin()
        for a, b in zip(cuts, cuts[1:]):
            _packed(eng, 0 if b <= 1000 or len(cuts) == 2 else 1, p.reads[a:b])
        eng.sample_finalize(1 if len(cuts) == 2 else 2)
        _check(eng, p.placed, p.regs_a, p.table_a, what=len(cuts))
        _check(eng, p.placed, p.regs_b, p.table_b, what=("30 / 10", len(cuts)))


def test_again_with_other_regions_no_regions_and_a_small_cap(world):
    p, eng = world.p, world.eng
    _sample(eng, p.reads)
    _check(eng, p.placed, p.regs_b, p.table_b)
    _check(eng, p.placed, p.regs_a, p.table_a)                                         # fewer regions: the old table is zeroed, not added to
    _check(eng, p.placed, [], ([], [], []), what="no regions")
    summ, cover, ref, entries = eng.download_haplotypes(cap=3)
    assert (len(cover), len(ref), entries, summ.entries) == (0, 0, [], 0)
    _check(eng, p.placed, p.regs_a, p.table_a)
    summ, cover, ref, entries = eng.download_haplotypes(cap=7)                         # fewer than there are: `cap` entries, the full count
    assert summ.entries == len(p.table_a[2]) and entries == p.table_a[2][:7]
    raw, s2 = np.full((12, 40), 0xff, np.uint8), _ffi.HapSummary()
    assert eng._L.bk_sample_download_haplotypes(eng.h, C.byref(s2), None, None, raw.ctypes.data_as(C.c_void_p), 5) == 0
    assert (raw[5:] == 0xff).all() and not (raw[:5] == 0xff).all()                     # the entries beyond cap are untouched
    assert eng._L.bk_sample_download_haplotypes(eng.h, None, None, None, None, 0) == -1
    assert eng._L.bk_sample_download_haplotypes(eng.h, C.byref(s2), None, None, None, 3) == -1


@pytest.mark.parametrize("order", ["haplotypes_last", "haplotypes_first"])
def test_linkage_codons_and_haplotypes_on_one_sample(world, order):
    p, eng = world.p, world.eng
    sites = [codon_cases.SAMPLE_P + o for o in (0, 2, 30, 63, 64, 65, 100)]
    pairs = linkage_ref.link_count(p.g, p.rows, sites, 1000)
    regs = codons_ref.regions_of(p.genes)
    _sample(eng, p.reads)
    steps = [lambda: eng.sample_linkage(sites, 1000), lambda: eng.sample_codons(regs), lambda: eng.sample_haplotypes(p.regs_a, 12)]
    for step in (steps if order == "haplotypes_last" else steps[::-1]):
        step()
    for _ in range(2):
        summ, got = eng.download_linkage()
        assert got == pairs and summ.placed == p.placed
        assert np.array_equal(eng.download_codons()[1], p.gene_counts)
        summ, cover, ref, entries = eng.download_haplotypes()
        assert (list(cover), list(ref), entries) == p.table_a and summ.rows == p.placed
        eng.sample_haplotypes(p.regs_a, 10)                                            # ... and again: the others' counters stay


def test_eight_mismatches_on_both_strands_through_every_reader_of_the_store(world):
    """A row's codec at its limits: a record along and one against the reference, each with all eight mismatch slots in use (the second
    found from its last cell down, each put in front), the first and the last of them on the first and last cell of a region.  The rows
    are downloaded, then linkage, codons and haplotypes are counted on that one sample: everything equal to the restatements."""
    p, eng = world.p, world.eng
    start, offs = haplotype_cases.HOT_START, [40 + 9 * t for t in range(8)]
    fwd = indel_cases.mut_read(p.g.text, start, 150, subs=tuple(offs))
    reads = [fwd, indels_ref.revcomp(indel_cases.mut_read(p.g.text, start + 3, 150, subs=tuple(o - 3 for o in offs[:4]) + tuple(o - 1 for o in offs[4:])))]
    rows, t = linkage_ref.link_rows(p.g, reads, 8)
    assert t["placed"] == 2 and sorted(r[2] for r in rows) == [0, 1] and all(len(r[3]) == 8 for r in rows), (t, rows)
    first, last = start + offs[0], start + offs[-1] + 2                                # the first mismatch of both rows, the last of the second
    assert all(r[0] + r[3][0][0] == first for r in rows) and max(r[0] + r[3][-1][0] for r in rows) == last
    _sample(eng, reads)
    assert eng.download_link_rows() == rows
    sites = sorted({r[0] + o for r in rows for o, _ in r[3]} | {first - 1, last + 1})
    eng.sample_linkage(sites, 1000)
    summ, pairs = eng.download_linkage()
    assert pairs == linkage_ref.link_count(p.g, rows, sites, 1000) and (summ.placed, summ.discordant) == (2, 0)
    regs = [(first - f, (last - first + f) // 3 + 1) for f in range(3)]               # the three frames: each holds the first and the last mismatch
    eng.sample_codons(regs)
    assert np.array_equal(eng.download_codons()[1], codons_ref.codon_count(p.g, rows, regs))
    hregs = [(first, last + 1 - first), (first + 1, last - 1 - first), (first, offs[-1] - offs[0] + 1), (start, 150)]
    cover, ref, entries = _check(eng, 2, hregs, haplotypes_ref.hap_count(p.g, rows, hregs), what="eight on both strands")
    assert list(cover) == [2, 2, 2, 1] and list(ref) == [0, 0, 0, 0] and sorted(len(h) for r, _, h in entries if r == 0) == [8, 8]


def test_an_engine_its_fork_and_a_store_that_grew(world):
    p = world.p
    fork = world.eng.fork()
    try:
        _sample(fork, p.reads[:100])                                # a fork has no row store of its parent's
        with pytest.raises(BronkoError) as ei:
            fork.sample_haplotypes(p.regs_a)
        assert ei.value.status == -5
        fork.linkage_enable(8, 16)                                  # 16 rows, 2,000 records, four pushes
        fork.sample_begin()
        for a, b in ((0, 37), (37, 700), (700, 1301), (1301, 2000)):
            _packed(fork, 0, p.reads[a:b])
        fork.sample_finalize(1)
        _check(fork, p.placed, p.regs_a, p.table_a, what="grown store")
        for e, n in ((world.eng, 2000), (fork, 500), (world.eng, 1000)):
            _one(e, p.g, p.reads[:n], 8, p.regs_a, what=n)
    finally:
        fork.close()


def test_call_order_and_parameters(world):
    p = world.p
    eng = world.ix.engine()

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        assert status(eng.sample_haplotypes, p.regs_a)[0] == -5       # linkage is not enabled
        eng.linkage_enable()
        assert status(eng.sample_haplotypes, p.regs_a)[0] == -5       # nothing was ever begun
        assert status(eng.download_haplotypes)[0] == -5
        eng.sample_begin()
        assert status(eng.sample_haplotypes, p.regs_a)[0] == -5       # inside a sample
        _packed(eng, 0, p.reads[:300])
        assert status(eng.sample_haplotypes, p.regs_a)[0] == -5       # before the finalize
        eng.sample_finalize(1)
        rows, t = linkage_ref.link_rows(p.g, p.reads[:300], 8)
        summ, cover, ref, entries = eng.download_haplotypes()         # before the first count: the rows and no regions
        assert (summ.rows, summ.n_regions, summ.entries, len(cover), entries) == (t["placed"], 0, 0, 0, [])
        cells = p.g.cells
        for bad, word in (([(5, 3), (9, 0)], "region 1"), ([(0, 1), (5, 2), (cells - 5, 6)], "region 2"), ([(cells, 1)], "region 0"), ([(0, 65521)], "65521"),
                          ([(0, 1)] * 4097, "4097")):
            st, msg = status(eng.sample_haplotypes, bad)
            assert st == -1 and word in msg, (bad[:3], msg)
        for log2 in (9, 25, 0):
            st, msg = status(eng.sample_haplotypes, p.regs_a, log2)
            assert st == -1 and "table_log2" in msg, msg
        summ, cover, ref, entries = eng.download_haplotypes()         # no launch was made, nothing was counted
        assert (summ.rows, summ.n_regions, entries) == (t["placed"], 0, [])
        want = haplotypes_ref.hap_count(p.g, rows, p.regs_a)
        _check(eng, t["placed"], p.regs_a, want)                      # needs the finalize only, not bk_sample_call
        _check(eng, t["placed"], [(0, 65520 if cells >= 65520 else cells)], ([0], [0], []), what="a region longer than any read")
        eng.sample_call(1)
        _check(eng, t["placed"], p.regs_a, want, log2=24)             # ... and after the call as well; the largest table
        assert status(eng.sample_haplotypes, [(5, 0)])[0] == -1
        assert eng.download_haplotypes()[3] == want[2]                # a refused call leaves the last table alone
        eng.sample_begin()                                            # the next sample: nothing is this sample's yet
        assert status(eng.download_haplotypes)[0] == -5 and status(eng.sample_haplotypes, p.regs_a)[0] == -5
        eng.sample_finalize(1)
        summ, cover, ref, entries = eng.download_haplotypes()
        assert (summ.rows, summ.n_regions, entries) == (0, 0, [])
        _check(eng, 0, p.regs_a, ([0] * len(p.regs_a), [0] * len(p.regs_a), []), what="an empty sample")
        eng.linkage_enable(None)                                      # the table goes with the row store
        assert status(eng.download_haplotypes)[0] == -5
    finally:
        eng.close()
    seqs = indel_cases.crafted_genome(K)                              # two sequences: a region across their border
    ix2 = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in seqs])])
    eng2 = ix2.engine()
    try:
        eng2.linkage_enable()
        _sample(eng2, [seqs[0][1][900:1050]])
        n_a = len(seqs[0][1])
        st, msg = status(eng2.sample_haplotypes, [(n_a - 30, 30), (n_a - 3, 5)])
        assert st == -1 and "region 1" in msg and "border" in msg, msg
        eng2.sample_haplotypes([(n_a - 30, 30), (n_a, 5)])
    finally:
        eng2.close()
        ix2.close()


def test_every_other_result_is_the_same_and_nothing_is_allocated_without_the_call(world):
    p = world.p
    plain, used = world.ix.engine(), world.ix.engine()
    sites = [codon_cases.SAMPLE_P + o for o in (0, 2, 30, 63)]
    try:
        out = []
        for eng in (plain, used):
            eng.linkage_enable(8, 4096)
            free = []
            for rep in range(3):
                eng.sample_begin()
                _packed(eng, 0, p.reads[:1000])
                _packed(eng, 1, p.reads[1000:])
                res = eng.sample_finish(2)
                if eng is used:
                    eng.sample_haplotypes(p.regs_a, 12)
                    assert eng.download_haplotypes()[3] == p.table_a[2]
                eng.sample_call(2)
                summ, recs = eng.download_calls()
                eng.sample_linkage(sites, 1000)
                eng.sample_codons(p.frames[:1])
                free.append(device_memory(0)[0])
            # an engine that never counts haplotypes allocates nothing after its first sample; one that does, nothing after its first count
            assert free[1] == free[0] and free[2] == free[0], (eng is used, free)
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        eng.download_linkage()[1], eng.download_link_rows(), eng.download_codons()[1].tobytes()))
        for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
            assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
        assert out[0][1:] == out[1][1:] and out[0][1][1] > 0 and len(out[0][3]) == 6    # (the same calls, pairs, rows and codons; the sample has calls)
    finally:
        plain.close()
        used.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_haplotypes_end_to_end(world, tmp_path, paired):
    p = world.p
    reads = _b(p.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        path = str(tmp_path / ("hap_R%d.fastq.gz" % (m + 1)))
        with gzip.open(path, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(path)
    bed = str(tmp_path / "amplicons.bed")
    named = [(2050, 100, "ampA"), (1940, 150, ""), (2000, 66, "ampC"), (100, 7000, "long"), (2050, 100, "again"), (3400, 120, "ampF")]
    with open(bed, "w") as f:
        f.write("# chrom\tstart\tend\tname\n")
        for start, ln, name in named:
            f.write("HPV16REF\t%d\t%d\t%s\t0\t-\n" % (start, start + ln, name))
    genes = str(tmp_path / "genes.bed")
    with open(genes, "w") as f:
        for c0, nc, _, start, strand, name in p.genes:
            f.write("HPV16REF\t%d\t%d\t%s\t0\t%s\n" % (start, start + 3 * nc, "" if name == "." else name, strand))
    wins = haplotypes_ref.read_bed(p.g, bed)
    assert [w[4] for w in wins] == ["ampA", ".", "ampC", "long", "again", "ampF"]
    # the testing build of the engine in the release build's place: BK_HAP_TABLE_SHRINK makes the first table one of 2^10 slots
    libs = tmp_path / "testing_lib"
    libs.mkdir()
    os.symlink(os.path.join(ROOT, "bronko_amd", "libbronko_hip_testing.so"), str(libs / "libbronko_hip.so"))
    small = dict(os.environ, BK_HAP_TABLE_SHRINK="6", LD_LIBRARY_PATH=str(libs) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs, logs = {}, {}
    for name, extra, env in (("bed", ["--haplotypes", bed], None), ("strict", ["--haplotypes", bed, "--hap-max-mismatches", "3", "--hap-min-reads", "20", "--hap-min-freq", "0.5"], None),
                             ("windows", ["--hap-window", "100", "--hap-step", "50"], None), ("tiles", ["--hap-window", "30", "--hap-step", "10"], None),
                             ("tiles_small", ["--hap-window", "30", "--hap-step", "10"], small), ("windows_small", ["--hap-window", "100", "--hap-step", "50"], small),
                             ("all", ["--haplotypes", bed, "--linkage", "--codons", genes], None), ("others", ["--linkage", "--codons", genes], None), ("without", [], None)):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("distinct haplotypes" in res.stdout) == ("--haplotypes" in extra or "--hap-window" in extra)
        outs[name], logs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}, res.stdout
    stem = "hap_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    # a table that was full is counted again with four times the slots; one that was not, is not
    assert "2^10 slots was full" in logs["tiles_small"] and "table of 2^12 slots" in logs["tiles_small"]
    assert "was full" not in logs["windows_small"] and "table of 2^10 slots" in logs["windows_small"]
    assert "was full" not in logs["tiles"] and "table of 2^16 slots" in logs["tiles"]
    assert "%d placed records over 788 regions" % p.placed in logs["tiles"]
    seen = set()
    for name, w, (M, N, F) in (("bed", wins, (8, 5, 0.03)), ("strict", wins, (3, 20, 0.5)), ("windows", p.wins_a, (8, 5, 0.03)), ("tiles", p.wins_b, (8, 5, 0.03)),
                               ("tiles_small", p.wins_b, (8, 5, 0.03)), ("windows_small", p.wins_a, (8, 5, 0.03)), ("all", wins, (8, 5, 0.03))):
        base = "others" if name == "all" else "without"
        assert set(outs[name]) == set(outs[base]) | {stem + ".haplotypes.tsv"}
        for f in outs[base]:                                       # every other output does not know of the flag
            assert outs[name][f] == outs[base][f], (name, f)
        rows = p.rows if M == 8 else linkage_ref.link_rows(p.g, p.reads, M)[0]
        table = haplotypes_ref.hap_count(p.g, rows, haplotypes_ref.regions_of(w))
        want = haplotypes_ref.tsv_text(p.g, w, *table, M, N, F)
        assert want.count("\n") >= 5                                # four header lines and at least one haplotype
        assert outs[name][stem + ".haplotypes.tsv"].decode() == want, name
        lines, no_cover, distinct = haplotypes_ref.stats(*table, want)
        assert "%d without cover, %d distinct haplotypes, %d lines written" % (no_cover, distinct, lines) in logs[name], logs[name]
        seen.add(want)
    assert len(seen) == 4
