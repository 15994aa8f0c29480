"""`bronko call --linkage` without a GPU: the host twin (bronko_amd/host/linkage.cpp through bh_link_rows / bh_link_count) against
the Python restatement of the rule (tests/linkage_ref.py) -- rows as multisets, every counter of every pair, the tallies, the TSV
text byte for byte --, the restatement itself against what was planted, and the argument errors of `bronko call`."""
import os
import subprocess

import pytest

from bronko_amd import hostlib
from bronko_amd.engine import link_rows as decode_rows
from bronko_amd.hostlib import HostIndex
from tests import indel_cases, indels_ref, linkage_cases, linkage_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
CODE = linkage_ref._CODE


def _both(ix, g, reads, sites, M=8, D=1000):
    """The twin's and the restatement's rows, tallies and counters of the same reads; asserts that they are equal."""
    raw, counters = hostlib.link_rows(ix, 0, reads, M)
    rows, t = linkage_ref.link_rows(g, reads, M)
    got = decode_rows(raw)
    assert got == rows, ("rows", [r for r in got if r not in rows][:3], [r for r in rows if r not in got][:3])
    assert counters == (t["records"], t["placed"], t["unplaced"], t["discordant"])
    pairs = linkage_ref.link_count(g, rows, sites, D)
    assert hostlib.link_count(ix, 0, raw, sites, D) == pairs
    return rows, t, pairs, raw


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    yield k, ix, g, linkage_cases.crafted_cases(k), linkage_cases.crafted_sites(k)
    ix.close()


@pytest.fixture(scope="module")
def planted():
    return linkage_cases.Planted()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases, sites = crafted
    reads = [r for _, r in cases]
    for M in (0, 2, 8):
        rows, t, pairs, _ = _both(ix, g, reads, sites, M)
        assert t["placed"] > 4 and t["discordant"] > 0 and t["unplaced"] > 0
        assert t["records"] == t["placed"] + t["unplaced"] + t["discordant"]
    _both(ix, g, reads, sites, 8, 2)                                # only the closest sites pair up
    _both(ix, g, reads, sites, 8, 65519)
    for label, read in cases:                                      # ... and one by one, so that a difference names its record
        _both(ix, g, [read], sites)


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone."""
    k, ix, g, cases, sites = crafted
    first_b, S, n = g.first[1], linkage_cases.START, linkage_cases.N_LEN
    by = {label: linkage_ref.link_rows(g, [read], 8) for label, read in cases}
    for label, (rows, t) in by.items():
        base = label.split("/")[0]
        strand = 1 if label.endswith("/rc") else 0
        if base in ("deletion", "over_N", "across_sequences", "on_duplicate", "n_2k_minus_1", "mm_9", "step_bounds"):
            assert rows == [] and t["placed"] == 0, label
            assert t["discordant"] == (1 if base == "mm_9" else 0), label
        elif base == "split_at_N":
            assert t["records"] == 2 and t["placed"] == 2, label
        else:
            assert len(rows) == 1 and rows[0][2] == strand, (label, t)
    assert [m[0] for m in by["ends"][0][0][3]] == [m[0] for m in by["ends/rc"][0][0][3]] == [0, n - 1]
    assert by["ends"][0][0][:2] == by["ends/rc"][0][0][:2] == (S, n)
    assert by["ends"][0][0][3] == by["ends/rc"][0][0][3]            # the bases are the reference orientation's on either strand
    assert [m[0] for m in by["step_15_16/rc"][0][0][3]] == [15, 16] and [m[0] for m in by["step_31_32"][0][0][3]] == [31, 32]
    assert [m[0] for m in by["step_47_64"][0][0][3]] == [m[0] for m in by["step_47_64/rc"][0][0][3]] == [47, 48, 63, 64]
    assert [m[0] for m in by["n_157"][0][0][3]] == [144, 156] and by["n_160/rc"][0][0][3][0][0] == 159
    for m in (1, 2, 3, 8):
        assert len(by["mm_%d" % m][0][0][3]) == m
        rows, t = linkage_ref.link_rows(g, [dict(cases)["mm_%d/rc" % m]], m - 1)   # one more than M: discordant
        assert rows == [] and t["discordant"] == 1
    assert by["second_seq"][0][0][0] == first_b + 100
    # the sites at a record's first and last cell are covered, the cells outside either end are not
    reads = [r for _, r in cases]
    rows, _ = linkage_ref.link_rows(g, reads, 8)
    pairs = {(a, b): c for a, b, c in linkage_ref.link_count(g, rows, sites, 1000)}
    assert sum(pairs[(S, S + n - 1)]) > 20
    assert sum(pairs[(S - 1, S)]) == 0 and sum(pairs[(S + n - 1, S + n)]) == 4   # (only the records of 157 and 160 bases reach S + n)
    a72 = pairs[(S + 70, S + 72)]
    r70, r72 = CODE[g.text[S + 70]], CODE[g.text[S + 72]]
    assert a72[4 * ((r70 + 1) % 4) + (r72 + 1) % 4] == 2 and a72[4 * ((r70 + 1) % 4) + r72] == 2   # apart_2 and apart_5, either strand
    assert not any((a < first_b) != (b < first_b) for a, b in pairs)                               # no pair crosses sequences
    assert sum(pairs[(first_b + 110, first_b + 150)]) == 4
    assert (g.first[1] - 1, first_b) not in pairs and (g.first[1] - 5, first_b - 1) in pairs


def test_planted_sample_twin_equals_restatement(planted):
    p = planted
    ix = HostIndex.build(p.k, [linkage_cases.HPV])
    try:
        rows, t, pairs, raw = _both(ix, p.g, p.reads, p.sites)
        assert rows == p.rows and pairs == p.pairs
        every = list(range(2000, 2400))                            # many sites in one row
        assert hostlib.link_count(ix, 0, raw, every, 1000) == linkage_ref.link_count(p.g, rows, every, 1000)
        _both(ix, p.g, p.reads[:500], p.sites, 2, 100)
        with pytest.raises(RuntimeError):
            hostlib.link_count(ix, 0, raw, [5, 5], 1000)
        with pytest.raises(RuntimeError):
            hostlib.link_count(ix, 0, raw, [7, 5], 1000)
        with pytest.raises(RuntimeError) as ei:                    # 1,500 sites within 1,000 cells of each other: more than 2^20 pairs
            hostlib.link_count(ix, 0, raw, list(range(1000, 2500)), 65519)
        assert "pairs" in str(ei.value)
    finally:
        ix.close()


def test_planted_sample_is_not_vacuous(planted):
    """The restatement alone: haplotype 1's substitutions travel together, haplotype 2's never ride with them."""
    p = planted
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    by = {(a, b): c for a, b, c in p.pairs}

    def cell(a, b, alt_a, alt_b):
        ta, tb = p.g.text[a], p.g.text[b]
        return by[(a, b)][4 * CODE[nxt[ta] if alt_a else ta] + CODE[nxt[tb] if alt_b else tb]]

    h1, h2 = p.hap1, p.hap2
    for a, b in ((h1[0], h1[1]), (h1[0], h1[2]), (h1[1], h1[2])):
        assert cell(a, b, 1, 1) > 20 and cell(a, b, 0, 0) > 5 and cell(a, b, 1, 0) + cell(a, b, 0, 1) <= 4, (a, b, by[(a, b)])
    a, b = h1[2], h1[3]                                            # 140 apart: only records that begin within ten cells cover both
    assert cell(a, b, 1, 1) > 0 and cell(a, b, 1, 0) + cell(a, b, 0, 1) <= 1, by[(a, b)]
    assert sum(by[(h1[0], h1[3])]) == 0                             # 203 apart: no record of 150 bases covers both
    assert (h1[0], h1[4]) not in by                                # beyond max_dist
    a, b = h1[0], h2[0]                                            # repulsion: each alone, never both
    assert cell(a, b, 1, 1) == 0 and cell(a, b, 1, 0) > 20 and cell(a, b, 0, 1) > 5
    assert cell(h2[0], h2[1], 1, 1) > 5


def test_tsv_text(planted, tmp_path):
    p = planted
    ix = HostIndex.build(p.k, [linkage_cases.HPV])
    try:
        recs = p.recs + [(p.hap1[0], p.g.text[p.hap1[0]], "T" if p.g.text[p.hap1[0]] != "G" else "A")]   # a second record at one cell
        recs = [r for r in recs if r[1] != r[2]]
        coded = [(c, CODE[r], CODE[a]) for c, r, a in recs]
        seen = set()
        for M, D, N in ((8, 1000, 1), (8, 1000, 300), (2, 70, 1), (8, 1, 1)):
            rows, _ = linkage_ref.link_rows(p.g, p.reads, M)
            pairs = linkage_ref.link_count(p.g, rows, p.sites, D)
            want = linkage_ref.tsv_text(p.g, recs, pairs, M, D, N)
            path = str(tmp_path / ("l_%d_%d_%d.tsv" % (M, D, N)))
            lines = hostlib.write_linkage_tsv(path, ix, 0, coded, pairs, M, D, N)
            assert open(path).read() == want and lines == want.count("\n") - 4
            seen.add(lines)
        assert len(seen) >= 3 and 0 in seen                        # a sample without such a pair: the header alone
        assert want.startswith("##link_max_mismatches=8\n##link_max_dist=1\n##link_min_reads=1\nchrom\tpos_a\tref_a\talt_a\tpos_b\t")
        text = linkage_ref.tsv_text(p.g, recs, p.pairs)
        body = [ln.split("\t") for ln in text.splitlines()[4:]]
        assert [int(ln[1]) for ln in body] == sorted(int(ln[1]) for ln in body) and body[0][1] == str(p.hap1[0] + 1)
        assert all(int(ln[7]) == sum(int(v) for v in ln[8:]) for ln in body)
    finally:
        ix.close()


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--link-max-mismatches", "2"], "--linkage"), (["--link-max-dist", "10"], "--linkage"), (["--link-min-reads", "3"], "--linkage"),
                        (["--linkage", "--link-max-mismatches", "-1"], "--link-max-mismatches"), (["--linkage", "--link-max-mismatches", "9"], "--link-max-mismatches"),
                        (["--linkage", "--link-max-dist", "0"], "--link-max-dist"), (["--linkage", "--link-max-dist", "65520"], "--link-max-dist"),
                        (["--linkage", "--link-min-reads", "0"], "--link-min-reads")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    assert _run(*base, "--linkage", "--link-max-dist", "x").returncode == 2
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--linkage")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
