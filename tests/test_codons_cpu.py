"""`bronko call --codons` without a GPU: the host twin (bronko_amd/host/codons.cpp through bh_codon_count, bh_codon_bed,
bh_write_codons_tsv) against the Python restatement of the rule (tests/codons_ref.py) -- every counter of every codon, the BED
reader's genes and errors, the TSV text byte for byte --, the restatement's two ways to the table against each other, and the
argument errors of `bronko call`.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import codon_cases, codons_ref, indel_cases, indels_ref, linkage_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _both(ix, g, reads, regions, M=8):
    """The twin's and the restatement's counters of the same reads; asserts that they are equal."""
    raw, _ = hostlib.link_rows(ix, 0, reads, M)
    rows, _ = linkage_ref.link_rows(g, reads, M)
    want = codons_ref.codon_count(g, rows, regions)
    got = hostlib.codon_count(ix, 0, raw, regions)
    assert got.shape == want.shape and np.array_equal(got, want), [(i, got[i].nonzero(), want[i].nonzero()) for i in np.flatnonzero((got != want).any(axis=1))[:3]]
    return rows, want


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    yield k, ix, g, codon_cases.crafted_cases(k), codon_cases.crafted_regions(k)
    ix.close()


@pytest.fixture(scope="module")
def planted():
    return codon_cases.Planted()


@pytest.fixture(scope="module")
def hpv_ix():
    ix = HostIndex.build(21, [codon_cases.HPV])
    yield ix
    ix.close()


def _ref_triplet(g, cell):
    return sum("ACGT".index(c) << (4 - 2 * i) for i, c in enumerate(g.text[cell:cell + 3]))


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases, regions = crafted
    reads = [r for _, r in cases]
    for M in (0, 2, 8):
        rows, want = _both(ix, g, reads, regions, M)
        assert np.array_equal(codons_ref.codon_count_by_differences(g, rows, regions), want)
        other = sum(int(want[c].sum()) - int(want[c, _ref_triplet(g, c0 + 3 * i)])
                    for c, (c0, i) in enumerate((c0, i) for c0, nc in regions for i in range(nc)) if "N" not in g.text[c0 + 3 * i:c0 + 3 * i + 3])
        assert (other == 0) if M == 0 else (other > 50 if M == 8 else other > 10), (M, other)
    for label, read in cases:                                      # ... and one by one, so that a difference names its record
        _both(ix, g, [read], regions)
    _both(ix, g, reads, [])
    _both(ix, g, [], regions)


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on single crafted records."""
    k, ix, g, cases, regions = crafted
    S, by = codon_cases.START, dict(cases)
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}

    def table(label, regs, placed=1):
        rows, t = linkage_ref.link_rows(g, [by[label]], 8)
        assert t["placed"] == placed, (label, t)
        return rows[0], codons_ref.codon_count(g, rows, regs)

    for label in ("plain", "plain/rc"):                            # the three frames: 50, 49 and 49 codons lie wholly under the record
        _, c = table(label, regions[:3])
        assert [int(c[a:b].sum()) for a, b in ((0, 50), (50, 100), (100, 149))] == [50, 49, 49]
        assert int(c[99].sum()) == 0 and int(c[100].sum()) == 1    # the second frame's last codon ends one cell behind the record
    _, c = table("plain", [(S - 1, 20), (S + 121, 10), (S + 120, 10), (S, 10)])
    assert [int(x.sum()) for x in c[:2]] == [0, 1] and [int(x.sum()) for x in c[28:30]] == [1, 0] and int(c[39].sum()) == 1 and int(c[40].sum()) == 1
    for label in ("apart_2", "apart_2/rc"):                        # offsets 70 and 72: one codon of the second frame, two of the first
        _, c = table(label, [(S + 1, 50), (S, 50), (S + 70, 1)])
        alt = [nxt[ch] if i in (0, 2) else ch for i, ch in enumerate(g.text[S + 70:S + 73])]
        t = sum("ACGT".index(ch) << (4 - 2 * i) for i, ch in enumerate(alt))
        assert c[23, t] == 1 and c[100, t] == 1 and int(c[23].sum()) == 1
        assert c[50 + 23, _ref_triplet(g, S + 69)] == 0 and c[50 + 24, _ref_triplet(g, S + 72)] == 0 and int(c[50 + 23].sum()) == int(c[50 + 24].sum()) == 1
    for label in ("triple", "triple/rc"):                          # 90, 91, 92: all three letters of one codon of the first frame
        _, c = table(label, [(S, 50), (S + 1, 50)])
        t = sum("ACGT".index(nxt[ch]) << (4 - 2 * i) for i, ch in enumerate(g.text[S + 90:S + 93]))
        assert c[30, t] == 1 and int(c[30].sum()) == 1
        assert c[50 + 29, _ref_triplet(g, S + 88)] == 0 and c[50 + 30, _ref_triplet(g, S + 91)] == 0
    for label, cells in (("step_15_16", (15, 16)), ("step_31_32", (31, 32))):
        _, c = table(label, regions[:3])
        changed = [int(np.count_nonzero([c[ci, _ref_triplet(g, c0 + 3 * i)] == 0 and c[ci].sum() == 1 for i in range(nc) for ci in [b + i]]))
                   for b, (c0, nc) in zip((0, 50, 100), regions[:3])]
        assert sorted(changed) == [1, 1, 2], (label, changed)       # one codon in two of the frames, neighbouring codons in the third
    _, c = table("split_at_N", [(1290, 15)], placed=2)              # a record either side of the N
    assert [int(x.sum()) for x in c] == [1] * 3 + [0] * 7 + [1] * 5 # a codon that holds an N lies under no row
    _, c = table("end_of_first", [(len(g.seqs[0]) - 30, 10)])
    assert [int(x.sum()) for x in c] == [1] * 10
    _, c = table("second_seq", [(len(g.seqs[0]) + 100, 40), (len(g.seqs[0]) + 101, 30)])
    assert int(c[:40].sum()) == 40 and int(c[40:].sum()) == 30


def test_planted_sample_twin_equals_restatement_and_both_ways_agree(planted, hpv_ix):
    p = planted
    raw, _ = hostlib.link_rows(hpv_ix, 0, p.reads, 8)
    assert np.array_equal(hostlib.codon_count(hpv_ix, 0, raw, p.frames), p.counts)
    assert np.array_equal(codons_ref.codon_count_by_differences(p.g, p.rows, p.frames), p.counts)
    regs = codons_ref.regions_of(p.genes)
    assert np.array_equal(hostlib.codon_count(hpv_ix, 0, raw, regs), p.gene_counts)
    assert np.array_equal(codons_ref.codon_count_by_differences(p.g, p.rows, regs + regs[::-1]), np.concatenate([p.gene_counts, codons_ref.codon_count(p.g, p.rows, regs[::-1])]))
    assert (p.tallies["placed"], p.double, p.triple) == (1955, 108, 99)
    for bad, word in (([(5, 0)], "region 0"), ([(0, 1), (p.g.cells - 2, 1)], "region 1"), ([(0, 1)] * 4097, "4097"), ([(0, 2600)] * 101, "262600")):
        with pytest.raises(RuntimeError) as ei:
            hostlib.codon_count(hpv_ix, 0, raw, bad)
        assert word in str(ei.value), (bad[:2], str(ei.value))


def test_a_minus_region_is_the_plus_region_mirrored_and_complemented(planted, hpv_ix, tmp_path):
    """The device counts forward-strand triplets only: a '-' line of the BED has the '+' line's counters, and the writer reads them
    from the last codon to the first with every triplet reverse-complemented."""
    p = planted
    bed = str(tmp_path / "pm.bed")
    open(bed, "w").write("HPV16REF\t1940\t2390\tfwd\t0\t+\nHPV16REF\t1940\t2390\trev\t0\t-\n")
    genes = hostlib.codon_bed(hpv_ix, 0, bed)
    assert genes == codons_ref.read_bed(p.g, bed) and [g[4] for g in genes] == ["+", "-"]
    counts = codons_ref.codon_count(p.g, p.rows, codons_ref.regions_of(genes))
    assert np.array_equal(counts[:150], counts[150:]) and counts.sum() > 1000
    body = [ln.split("\t") for ln in codons_ref.tsv_text(p.g, genes, counts).splitlines()[4:]]
    plus, minus = [ln for ln in body if ln[2] == "+"], [ln for ln in body if ln[2] == "-"]
    assert len(plus) == len(minus) > 3
    rc = lambda s: "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(s))
    mirrored = sorted((150 + 1 - int(ln[3]), ln[4], rc(ln[5]), rc(ln[7]), ln[9], ln[10], ln[11]) for ln in minus)
    assert mirrored == sorted((int(ln[3]), ln[4], ln[5], ln[7], ln[9], ln[10], ln[11]) for ln in plus)
    assert all(ln[6] == codons_ref.translate(ln[5]) and ln[8] == codons_ref.translate(ln[7]) for ln in body)
    assert all(hostlib.translate(t) == aa for t, aa in codons_ref.CODE.items()) and hostlib.translate("ANG") == "X"


def test_bed_reader_and_its_errors(planted, hpv_ix, tmp_path):
    p = planted

    def bed(name, text):
        path = str(tmp_path / name)
        open(path, "w").write(text)
        return path

    ok = bed("ok.bed", "# genes\ntrack name=x\nHPV16REF\t2000\t2300\tgeneA\t0\t+\n\nHPV16REF\t1940\t2390\tgeneB\t0\t-\nHPV16REF\t2001\t2121\nHPV16REF\t3\t9\t\t0\t.\r\n")
    genes = hostlib.codon_bed(hpv_ix, 0, ok)
    assert genes == codons_ref.read_bed(p.g, ok)
    assert genes == [(2000, 100, 0, 2000, "+", "geneA"), (1940, 150, 0, 1940, "-", "geneB"), (2001, 40, 0, 2001, "+", "."), (3, 2, 0, 3, "+", ".")]
    assert [r[:4] for r in hostlib.bed_regions(hpv_ix, ok)] == [(0, 0, 2000, 2300), (0, 0, 1940, 2390), (0, 0, 2001, 2121), (0, 0, 3, 9)]
    cases = [("len.bed", "HPV16REF\t0\t30\tg\t0\t+\nHPV16REF\t100\t131\th\t0\t+\n", "line 2", "multiple of 3"),
             ("chrom.bed", "HPV16REF\t0\t30\nHPV18\t0\t30\n", "line 2", "HPV18"),
             ("strand.bed", "HPV16REF\t0\t30\tg\t0\t*\n", "line 1", "strand"),
             ("end.bed", "HPV16REF\t7800\t8100\n", "line 1", "beyond"),
             ("many.bed", "".join("HPV16REF\t%d\t%d\n" % (i, i + 3) for i in range(4097)), "4097", "regions"),
             ("codons.bed", "HPV16REF\t0\t7800\n" * 101, "262600", "codons")]
    for name, text, where, word in cases:
        path = bed(name, text)
        with pytest.raises(RuntimeError) as ei:
            hostlib.codon_bed(hpv_ix, 0, path)
        assert path in str(ei.value) and where in str(ei.value) and word in str(ei.value), str(ei.value)
        with pytest.raises(ValueError):
            codons_ref.read_bed(p.g, path)
    # --regions reads the same files and never looks at column 6
    assert len(hostlib.bed_regions(hpv_ix, bed("strand2.bed", "HPV16REF\t0\t31\tg\t0\t*\textra\n"))) == 1


def test_tsv_text(planted, hpv_ix, tmp_path):
    p = planted
    seen = set()
    for M, N, F in ((8, 5, 0.03), (8, 1, 0.0), (8, 1, 1.0), (8, 100, 0.5), (8, 5, 0.6708), (8, 5, 0.6709), (2, 5, 0.03), (8, 4000, 0.0)):
        rows, _ = linkage_ref.link_rows(p.g, p.reads, M)
        counts = codons_ref.codon_count(p.g, rows, codons_ref.regions_of(p.genes))
        want = codons_ref.tsv_text(p.g, p.genes, counts, M, N, F)
        path = str(tmp_path / ("c_%d_%d_%g.tsv" % (M, N, F)))
        lines = hostlib.write_codons_tsv(path, hpv_ix, 0, p.genes, counts, M, N, F)
        assert open(path).read() == want and lines == want.count("\n") - 4, (M, N, F)
        seen.add(lines)
    assert len(seen) >= 5 and 0 in seen                            # a sample without such a line: the header lines alone
    assert want == "##codon_max_mismatches=8\n##codon_min_reads=4000\n##codon_min_freq=0\n" + "\t".join(codons_ref.HEADER) + "\n"
    text = codons_ref.tsv_text(p.g, p.genes, p.gene_counts)
    body = [ln.split("\t") for ln in text.splitlines()[4:]]
    assert body[0] == ["HPV16REF", "geneA", "+", "1", "2001", "TGC", "C", "AGG", "R", "108", "161", "0.6708", "missense"]
    assert {ln[12] for ln in body} == {"missense", "synonymous", "nonsense", "stop_lost"}
    assert [ln[1] for ln in body] == sorted((ln[1] for ln in body), key=["geneA", "geneB", ".", "geneD"].index)
    # count >= F * cover, the one floating product: 108 of 161 is written at 0.6708 and not at 0.6709
    at = [codons_ref.tsv_text(p.g, p.genes[:1], p.gene_counts[:100], 8, 5, F).count("\t108\t161\t") for F in (0.6708, 0.6709)]
    assert at == [1, 0]


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    ok = str(tmp_path / "ok.bed")
    open(ok, "w").write("HPV16REF\t2000\t2300\tgeneA\t0\t+\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    bad_len, bad_chrom = str(tmp_path / "len.bed"), str(tmp_path / "chrom.bed")
    open(bad_len, "w").write("HPV16REF\t2000\t2301\n")
    open(bad_chrom, "w").write("HPV16REF\t0\t30\nnowhere\t0\t30\n")
    for extra, words in ((["--codon-min-reads", "2"], ["--codons"]), (["--codon-min-freq", "0.1"], ["--codons"]), (["--codon-max-mismatches", "3"], ["--codons"]),
                         (["--codons", ok, "--codon-min-reads", "0"], ["--codon-min-reads"]), (["--codons", ok, "--codon-min-freq", "1.5"], ["--codon-min-freq"]),
                         (["--codons", ok, "--codon-min-freq", "-0.1"], ["--codon-min-freq"]),
                         (["--codons", ok, "--codon-max-mismatches", "9"], ["--codon-max-mismatches"]), (["--codons", ok, "--codon-max-mismatches", "-1"], ["--codon-max-mismatches"]),
                         (["--codons", ok, "--linkage", "--link-max-mismatches", "3"], ["--link-max-mismatches (3)", "--codon-max-mismatches (8)"]),
                         (["--codons", ok, "--linkage", "--codon-max-mismatches", "2"], ["--link-max-mismatches (8)", "--codon-max-mismatches (2)"]),
                         (["--codons", bad_len], [bad_len, "line 1", "multiple of 3"]), (["--codons", bad_chrom], [bad_chrom, "line 2", "nowhere"]),
                         (["--codons", str(tmp_path / "missing.bed")], ["missing.bed"])):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and all(w in r.stdout for w in words) and "no HIP device" not in r.stdout, (extra, r.stdout)
    assert _run(*base, "--codons", ok, "--codon-min-reads", "x").returncode == 2
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--codons", ok)
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
