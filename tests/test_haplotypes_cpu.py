"""`bronko call --haplotypes` without a GPU: the host twin (bronko_amd/host/haplotypes.cpp through bh_hap_count, bh_hap_regions,
bh_write_haplotypes_tsv) against the Python restatement of the rule (tests/haplotypes_ref.py) -- cover, ref_count and every entry,
the regions of a BED file and of the tiling and their errors, the TSV text byte for byte --, what the crafted records are meant to
show, and the argument errors of `bronko call`.  Every comparison is exact."""
import os
import subprocess

import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import codon_cases, haplotype_cases, haplotypes_ref, indel_cases, indels_ref, linkage_ref
from tests.linkage_cases import N_LEN, START

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _both(ix, g, reads, regions, M=8):
    """The twin's and the restatement's table of the same reads; asserts that they are equal."""
    raw, _ = hostlib.link_rows(ix, 0, reads, M)
    rows, _ = linkage_ref.link_rows(g, reads, M)
    cover, ref, entries = haplotypes_ref.hap_count(g, rows, regions)
    got = hostlib.hap_count(ix, 0, raw, regions)
    assert (list(got[0]), list(got[1])) == (cover, ref)
    assert got[2] == entries, [x for x in zip(got[2], entries) if x[0] != x[1]][:3]
    assert all(c == r + sum(n for i2, n, _ in entries if i2 == i) for i, (c, r) in enumerate(zip(cover, ref)))
    return rows, (cover, ref, entries)


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    yield k, ix, g, haplotype_cases.crafted_cases(k), haplotype_cases.crafted_regions(k)
    ix.close()


@pytest.fixture(scope="module")
def planted():
    return haplotype_cases.planted()


@pytest.fixture(scope="module")
def hpv_ix():
    ix = HostIndex.build(21, [codon_cases.HPV])
    yield ix
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases, regions = crafted
    reads = [r for _, r in cases]
    for M in (0, 2, 8):
        _, (cover, ref, entries) = _both(ix, g, reads, regions, M)
        assert (len(entries) == 0) if M == 0 else (len(entries) > 30 if M == 8 else len(entries) > 10), (M, len(entries))
    _both(ix, g, reads, regions[::-1])
    for label, read in cases:                                      # ... and one by one, so that a difference names its record
        _both(ix, g, [read], regions)
    _both(ix, g, reads, [])
    _both(ix, g, [], regions)


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on single crafted records and small groups of them."""
    k, ix, g, cases, regions = crafted
    S, E, by = START, START + N_LEN, dict(cases)
    nxt = {"A": 1, "C": 2, "G": 3, "T": 0}

    def table(labels, regs, placed=None):
        rows, t = linkage_ref.link_rows(g, [by[x] for x in labels], 8)
        assert t["placed"] == (len(labels) if placed is None else placed), (labels, t)
        return haplotypes_ref.hap_count(g, rows, regs)

    # region edges: spanned from the first cell to the last, not one cell further on either side
    cover, ref, entries = table(["plain"], [(S, N_LEN), (S - 1, N_LEN + 1), (S, N_LEN + 1), (S, 10), (E - 10, 10), (S - 1, 10), (E - 9, 10)])
    assert (cover, ref, entries) == ([1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 1, 1, 0, 0], [])
    # a substitution on the region's first and last cell is in the list, one just outside is not; eight inside one region
    for label in ("mm_8", "mm_8/rc"):
        cover, ref, entries = table([label], [(S + 40, 64), (S + 41, 62), (S + 41, 63), (S + 104, 20)])
        want = [(S + 40 + 9 * t, nxt[g.text[S + 40 + 9 * t]]) for t in range(8)]
        assert cover == [1] * 4 and ref == [0, 0, 0, 1]
        assert entries == [(0, 1, tuple((c - S - 40, b) for c, b in want)), (1, 1, tuple((c - S - 41, b) for c, b in want[1:7])),
                           (2, 1, tuple((c - S - 41, b) for c, b in want[1:]))]
    # rows that agree inside the region are one haplotype: whatever they carry outside it, whichever strand, first cell and length
    same = ["apart_2", "apart_2/rc", "apart_2_and_90", "apart_2_and_5/rc", "apart_2_longer", "shifted", "shifted/rc"]
    cover, ref, entries = table(same, [(S + 60, 20), (S, N_LEN), (S + 70, 1), (S + 71, 1)])
    hap = ((10, nxt[g.text[S + 70]]), (12, nxt[g.text[S + 72]]))
    assert cover == [7, 5, 7, 7] and ref == [0, 0, 0, 7]
    assert entries[0] == (0, 7, hap) and [e for e in entries if e[0] == 2] == [(2, 7, ((0, hap[0][1]),))]
    assert sorted(n for r, n, _ in entries if r == 1) == [1, 1, 3]   # over the whole record the two with a third substitution stand alone
    # a region over the N has no cover; one in the second sequence has its own offsets
    cover, ref, entries = table(["split_at_N", "second_seq", "second_seq_plain/rc"], [(1290, 40), (1250, 50), (len(g.seqs[0]) + 100, 60), (len(g.seqs[0]) + 105, 10)], placed=4)
    assert cover == [0, 1, 2, 2] and ref == [0, 1, 1, 1]
    assert entries == [(2, 1, ((10, nxt[g.text[len(g.seqs[0]) + 110]]), (50, nxt[g.text[len(g.seqs[0]) + 150]]))), (3, 1, ((5, nxt[g.text[len(g.seqs[0]) + 110]]),))]


def test_planted_sample_twin_equals_restatement(planted, hpv_ix):
    p = planted
    raw, _ = hostlib.link_rows(hpv_ix, 0, p.reads, 8)
    for regs, want in ((p.regs_a, p.table_a), (p.regs_b, p.table_b)):
        got = hostlib.hap_count(hpv_ix, 0, raw, regs)
        assert (list(got[0]), list(got[1]), got[2]) == want
    # the planted haplotypes: three substitutions in SAMPLE_P + 63 .. 65 together in most of the reads that span them
    i = p.regs_a.index((2050, 100))
    top = haplotypes_ref.ranked(p.table_a[0][i], p.table_a[1][i], [(c, h) for r, c, h in p.table_a[2] if r == i])
    assert [off for off, _ in top[0][1]] == [13, 14, 15] and top[0][0] > 20 and top[1][1] == ((50, ("ACGT".index(p.g.text[2100]) + 1) % 4),), top[:3]
    for bad, word in (([(5, 0)], "region 0"), ([(0, 1), (p.g.cells - 2, 3)], "region 1"), ([(0, 65521)], "65521"), ([(0, 1)] * 4097, "4097")):
        with pytest.raises(RuntimeError) as ei:
            hostlib.hap_count(hpv_ix, 0, raw, bad)
        assert word in str(ei.value), (bad[:2], str(ei.value))


def test_regions_of_a_bed_file_of_the_tiling_and_their_errors(planted, hpv_ix, tmp_path):
    p = planted

    def bed(name, text):
        path = str(tmp_path / name)
        open(path, "w").write(text)
        return path

    ok = bed("ok.bed", "# amplicons\ntrack name=x\nHPV16REF\t2000\t2300\tampA\t0\t-\n\nHPV16REF\t1940\t1941\nHPV16REF\t3\t9\t\t0\t*\textra\r\nHPV16REF\t2000\t2300\tagain\n")
    wins = hostlib.hap_regions(hpv_ix, 0, ok)
    assert wins == haplotypes_ref.read_bed(p.g, ok)
    assert wins == [(2000, 300, 0, 2000, "ampA"), (1940, 1, 0, 1940, "."), (3, 6, 0, 3, "."), (2000, 300, 0, 2000, "again")]   # strand is not looked at
    cases = [("chrom.bed", "HPV16REF\t0\t30\nHPV18\t0\t30\n", "line 2", "HPV18"),
             ("end.bed", "HPV16REF\t7800\t8100\n", "line 1", "beyond"),
             ("empty.bed", "HPV16REF\t30\t30\n", "line 1", "30"),
             ("many.bed", "".join("HPV16REF\t%d\t%d\n" % (i, i + 3) for i in range(4097)), "4097", "regions")]
    for name, text, where, word in cases:
        path = bed(name, text)
        with pytest.raises(RuntimeError) as ei:
            hostlib.hap_regions(hpv_ix, 0, path)
        assert path in str(ei.value) and where in str(ei.value) and word in str(ei.value), str(ei.value)
        with pytest.raises(ValueError):
            haplotypes_ref.read_bed(p.g, path)
    for W, S in ((100, 50), (30, 10), (100, 100), (7000, 1000), (p.g.cells, 1), (p.g.cells + 1, 1), (300, 7)):
        assert hostlib.hap_regions(hpv_ix, 0, None, W, S) == haplotypes_ref.windows(p.g, W, S), (W, S)
    assert hostlib.hap_regions(hpv_ix, 0, None, 100, 50) == p.wins_a and hostlib.hap_regions(hpv_ix, 0, None, p.g.cells + 1, 1) == []
    for W, S, word in ((0, 1, "window"), (65521, 1, "65521"), (100, 0, "step"), (100, 1, "7807")):
        with pytest.raises(RuntimeError) as ei:
            hostlib.hap_regions(hpv_ix, 0, None, W, S)
        assert word in str(ei.value), str(ei.value)


def test_two_sequences_are_tiled_each_on_its_own(crafted):
    k, ix, g, _, _ = crafted
    wins = hostlib.hap_regions(ix, 0, None, 400, 300)
    assert wins == haplotypes_ref.windows(g, 400, 300) and [(w[2], w[3]) for w in wins] == [(0, 0), (0, 300), (0, 600), (0, 900), (1, 0), (1, 300)]


def test_tsv_text(planted, hpv_ix, tmp_path):
    p = planted
    seen = set()
    for M, N, F in ((8, 5, 0.03), (8, 1, 0.0), (8, 1, 1.0), (8, 10, 0.5), (2, 5, 0.03), (8, 4000, 0.0)):
        table = p.table_a if M == 8 else haplotypes_ref.hap_count(p.g, linkage_ref.link_rows(p.g, p.reads, M)[0], p.regs_a)
        want = haplotypes_ref.tsv_text(p.g, p.wins_a, *table, M, N, F)
        path = str(tmp_path / ("h_%d_%d_%g.tsv" % (M, N, F)))
        got = hostlib.write_haplotypes_tsv(path, hpv_ix, 0, p.wins_a, *table, M, N, F)
        assert open(path).read() == want and got == haplotypes_ref.stats(*table, want), (M, N, F)
        seen.add(got[0])
    assert len(seen) >= 5 and 0 in seen                            # a sample without such a line: the header lines alone
    assert want == "##hap_max_mismatches=8\n##hap_min_reads=4000\n##hap_min_freq=0\n" + "\t".join(haplotypes_ref.HEADER) + "\n"
    text = haplotypes_ref.tsv_text(p.g, p.wins_a, *p.table_a)
    body = [ln.split("\t") for ln in text.splitlines()[4:]]
    assert [int(ln[1]) for ln in body] == sorted(int(ln[1]) for ln in body)                      # regions in the tiling's order
    assert all(int(ln[2]) - int(ln[1]) == 100 and ln[3] == "." and ln[0] == "HPV16REF" for ln in body)
    at = [ln for ln in body if ln[1] == "2050"]                     # ranked by count; freq truncated; positions 1-based in the sequence
    assert [int(ln[6]) for ln in at] == sorted(int(ln[6]) for ln in at) and [int(ln[7]) for ln in at] == sorted((int(ln[7]) for ln in at), reverse=True)
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    assert at[0][6] == "1" and at[0][9] == "3" and at[0][10] == ",".join("%d%s>%s" % (c + 1, p.g.text[c], nxt[p.g.text[c]]) for c in (2063, 2064, 2065))
    assert all(ln[8] == "%d.%04d" % divmod(10000 * int(ln[7]) // int(ln[4]), 10000) for ln in body) and any(ln[10] == "." for ln in body)
    # a BED file's names and a region without cover
    wins = [(2050, 100, 0, 2050, "ampA"), (100, 7000, 0, 100, "long"), (2050, 100, 0, 2050, "again")]
    table = haplotypes_ref.hap_count(p.g, p.rows, haplotypes_ref.regions_of(wins))
    want = haplotypes_ref.tsv_text(p.g, wins, *table)
    path = str(tmp_path / "named.tsv")
    assert hostlib.write_haplotypes_tsv(path, hpv_ix, 0, wins, *table) == haplotypes_ref.stats(*table, want) and open(path).read() == want
    names = [ln.split("\t")[3] for ln in want.splitlines()[4:]]
    assert table[0][1] == 0 and set(names) == {"ampA", "again"} and names.count("ampA") == names.count("again") == len(at)


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    ok = str(tmp_path / "ok.bed")
    open(ok, "w").write("HPV16REF\t2000\t2300\tampA\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    bad_chrom, bad_len, many = str(tmp_path / "chrom.bed"), str(tmp_path / "len.bed"), str(tmp_path / "many.bed")
    open(bad_chrom, "w").write("HPV16REF\t0\t30\nnowhere\t0\t30\n")
    open(bad_len, "w").write("HPV16REF\t0\t30\nHPV16REF\t0\t65521\n")
    open(many, "w").write("".join("HPV16REF\t%d\t%d\n" % (i, i + 3) for i in range(4097)))
    H = ["--haplotypes", ok]
    for extra, words in ((["--hap-min-reads", "2"], ["--haplotypes"]), (["--hap-min-freq", "0.1"], ["--haplotypes"]), (["--hap-max-mismatches", "3"], ["--haplotypes"]),
                         (["--hap-step", "5"], ["--hap-window"]), (H + ["--hap-step", "5"], ["--hap-window"]),
                         (H + ["--hap-window", "100"], ["--haplotypes", "--hap-window", "together"]),
                         (H + ["--hap-min-reads", "0"], ["--hap-min-reads"]), (H + ["--hap-min-freq", "1.5"], ["--hap-min-freq"]),
                         (H + ["--hap-min-freq", "-0.1"], ["--hap-min-freq"]),
                         (H + ["--hap-max-mismatches", "9"], ["--hap-max-mismatches"]), (H + ["--hap-max-mismatches", "-1"], ["--hap-max-mismatches"]),
                         (["--hap-window", "0"], ["--hap-window"]), (["--hap-window", "65521"], ["--hap-window", "65521"]),
                         (["--hap-window", "100", "--hap-step", "0"], ["--hap-step"]),
                         (["--hap-window", "100", "--hap-step", "1"], ["7807", "4096"]),
                         (H + ["--linkage", "--link-max-mismatches", "3"], ["--link-max-mismatches (3)", "--hap-max-mismatches (8)"]),
                         (H + ["--linkage", "--hap-max-mismatches", "2"], ["--link-max-mismatches (8)", "--hap-max-mismatches (2)"]),
                         (H + ["--codons", ok, "--codon-max-mismatches", "3"], ["--codon-max-mismatches (3)", "--hap-max-mismatches (8)"]),
                         (["--hap-window", "100", "--codons", ok, "--hap-max-mismatches", "2"], ["--codon-max-mismatches (8)", "--hap-max-mismatches (2)"]),
                         (["--haplotypes", bad_chrom], [bad_chrom, "line 2", "nowhere"]), (["--haplotypes", bad_len], [bad_len, "line 2", "65520"]),
                         (["--haplotypes", many], [many, "4097", "4096"]), (["--haplotypes", str(tmp_path / "missing.bed")], ["missing.bed"])):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and all(w in r.stdout for w in words) and "no HIP device" not in r.stdout, (extra, r.stdout)
    assert _run(*base, *H, "--hap-min-reads", "x").returncode == 2
    assert _run(*base, "--hap-window", "x").returncode == 2
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    for extra in (H, ["--hap-window", "100"]):
        r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
