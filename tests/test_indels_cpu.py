"""`bronko call --indels` without a GPU: the host twin (bronko_amd/host/indels.cpp through bh_indel_events) against the Python
restatement of the rule (tests/indels_ref.py) -- every event, every count, the whole span array --, the restatement itself against
what was planted, the report filter, the VCF text byte for byte, and the argument errors of `bronko call`."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import indel_cases, indels_ref
from tests.indels_ref import DEL, INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
HPV = os.path.join(ROOT, "tests", "golden", "HPV16.fa")


def _both(ix, g, reads, L=32, M=2):
    """The twin's and the restatement's (rows, span, counters) of the same reads; asserts that they are equal and returns them."""
    rows, span, counters = hostlib.indel_events(ix, 0, reads, L, M)
    res = indels_ref.indel_events(g, reads, L, M)
    want = indels_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    c = res.counters
    assert counters == (c["records"], c["anchored"], c["ref_spanning"], c["supporting"], c["discordant"])
    return res


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    yield k, ix, g, indel_cases.crafted_cases(k)
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for L, M in ((32, 0), (32, 2), (32, 4), (8, 8), (1, 2)):
        res = _both(ix, g, reads, L, M)
        assert res.events or L == 1
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the haplotype it supports, or nothing."""
    k, ix, g, cases = crafted
    for label, read, expect in cases:
        M = 4 if isinstance(expect, tuple) and expect[0] == "del4" else 2
        res = indels_ref.indel_events(g, [read], 32, M)
        against = label.endswith("/rc")
        if expect == "none":
            assert not res.events and not any(res.span), label
            if label.startswith("bp_in_last_k"):
                res0 = indels_ref.indel_events(g, [read], 32, 0)
                assert not res0.events and res0.counters["ref_spanning"] == 0, label
        elif expect == "span":
            assert not res.events and res.counters["ref_spanning"] >= 1 and sum(res.span_sums()) >= 1, label
        else:
            kind, cell, what = expect
            assert len(res.events) == 1, (label, res.events, res.counters)
            (ecell, ekind, elen, es), (fwd, rev) = next(iter(res.events.items()))
            assert (fwd, rev) == ((0, 1) if against else (1, 0)), label
            planted = (DEL, cell, what, "") if kind.startswith("del") else (INS, cell, len(what), what)
            assert ekind == planted[0] and elen == planted[2], label
            assert indel_cases.haplotype(g.text, ekind, ecell, elen, es) == indel_cases.haplotype(g.text, planted[0], planted[1], planted[2], planted[3]), label
            assert ecell <= cell, label                            # normalised to the left
            if kind == "delB":
                assert ecell == g.first[1] + 1, label              # the sequence's second cell
    by = {label: indels_ref.indel_events(g, [read]).events for label, read, _ in cases}
    assert list(by["homo_out"]) == list(by["homo_in"]) == [(300, DEL, 2, "")]
    assert list(by["dinuc_out"]) == list(by["dinuc_in"]) == [(500, INS, 2, "CA")]
    assert list(by["two_ins_0"])[0][:3] == list(by["two_ins_1"])[0][:3] and list(by["two_ins_0"]) != list(by["two_ins_1"])
    n2k = indels_ref.indel_events(g, [cases[[c[0] for c in cases].index("n_2k")][1]])
    assert sum(n2k.span_sums()) == 1                               # a record of 2k bases spans exactly one site
    split = indels_ref.indel_events(g, [cases[[c[0] for c in cases].index("n_splits")][1]])
    assert split.counters["records"] == 2 and split.counters["ref_spanning"] == 2
    all_reads = [r for _, r, _ in cases]
    res = indels_ref.indel_events(g, all_reads)
    two = [key for key in res.events if key[1] == INS and key[2] == 3]
    assert len(two) == 2 and two[0][0] == two[1][0] and all(res.events[key] == [1, 1] for key in two)


@pytest.fixture(scope="module")
def hpv_sample():
    g = {k: indels_ref.read_fasta(HPV, k) for k in (21, 31)}
    reads, planted = indel_cases.sample_reads(g[21].text)
    return g, reads, planted


@pytest.mark.parametrize("k", [21, 31])
def test_sample_twin_equals_restatement(hpv_sample, k):
    g, reads, planted = hpv_sample
    ix = HostIndex.build(k, [HPV])
    try:
        res = _both(ix, g[k], reads)
        assert res.counters["records"] == len(reads) and res.counters["supporting"] > 100
        _both(ix, g[k], reads[:300], 4, 0)
    finally:
        ix.close()


def test_sample_is_not_vacuous(hpv_sample):
    """The restatement alone finds every planted indel on both strands, with reference-spanning records at the four minor ones, and
    reports nothing that was not planted."""
    g, reads, planted = hpv_sample
    g = g[21]
    res = indels_ref.indel_events(g, reads)
    sums = res.span_sums()
    want = set()
    for kind, pos, what, af in planted:
        hap = indel_cases.haplotype(g.text, DEL if kind == "del" else INS, pos, what if kind == "del" else len(what), "" if kind == "del" else what)
        found = [key for key in res.events if indel_cases.haplotype(g.text, key[1], key[0], key[2], key[3]) == hap]
        assert len(found) == 1, (kind, pos)
        fwd, rev = res.events[found[0]]
        assert fwd >= 1 and rev >= 1, (kind, pos, fwd, rev)
        if af < 0.5:
            assert sums[found[0][0]] > 0, (kind, pos)
        want.add(found[0])
    reported = indels_ref.report(g, res, 5, 30000)
    assert reported and {r[:4] for r in reported} <= want
    assert {r[:4] for r in indels_ref.report(g, res, 1, 0)} == set(res.events)


def test_report_filter_and_vcf_text(hpv_sample, tmp_path):
    g, reads, planted = hpv_sample
    g = g[21]
    ix = HostIndex.build(21, [HPV])
    try:
        res = indels_ref.indel_events(g, reads)
        rows, span, _ = hostlib.indel_events(ix, 0, reads)
        seen = set()
        for min_reads in (1, 5):
            for ppm in (0, 30000, 1000000):
                want = indels_ref.report(g, res, min_reads, ppm)
                # the twin's filter is the engine's: support >= min_reads and support * 1e6 >= ppm * (support + ref_span), in integers
                mine = [r for r in rows if r[2] + r[3] >= min_reads and (r[2] + r[3]) * 1000000 >= ppm * (r[2] + r[3] + r[4])]
                assert [(r[0], abs(r[1]), r[2], r[3], r[4]) for r in mine] == [(w[0], w[2], w[4], w[5], w[6]) for w in want]
                seen.add(len(want))
                path = str(tmp_path / ("r%d_%d.indels.vcf" % (min_reads, ppm)))
                hostlib.write_indels_vcf(path, ix, 0, "reads/x.fastq", mine, 32, 2, min_reads, ppm)
                assert open(path).read() == indels_ref.vcf_text(g, want, indels_ref.vcf_header(g, "reads/x.fastq", 32, 2, min_reads, ppm))
        assert len(seen) >= 3                                      # the thresholds cut at different places
        path = str(tmp_path / "none.indels.vcf")                   # a sample without events: the header alone
        hostlib.write_indels_vcf(path, ix, 0, "", [], 7, 1, 5, 123456)
        text = open(path).read()
        assert text == indels_ref.vcf_text(g, [], indels_ref.vcf_header(g, "", 7, 1, 5, 123456)) and text.endswith("FILTER\tINFO\n")
        assert "##indel_min_af=0.123456\n" in text and "##indel_max_len=7\n" in text
    finally:
        ix.close()
    assert indels_ref.af_text(1, 2) == "0.3333" and indels_ref.af_text(3, 0) == "1.0000" and indels_ref.af_text(2, 1) == "0.6666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--indel-max-len", "8"], "--indels"), (["--indel-max-mismatches", "1"], "--indels"), (["--indel-min-reads", "3"], "--indels"),
                        (["--indel-min-af", "0.1"], "--indels"),
                        (["--indels", "--indel-max-len", "0"], "--indel-max-len"), (["--indels", "--indel-max-len", "33"], "--indel-max-len"),
                        (["--indels", "--indel-max-mismatches", "9"], "--indel-max-mismatches"), (["--indels", "--indel-min-reads", "0"], "--indel-min-reads"),
                        (["--indels", "--indel-min-af", "1.5"], "--indel-min-af"), (["--indels", "--indel-min-af", "-0.1"], "--indel-min-af")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--indels")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
