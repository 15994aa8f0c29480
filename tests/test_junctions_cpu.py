"""`bronko call --junctions` without a GPU: the host twin (bronko_amd/host/junctions.cpp through bh_junction_events) against the
Python restatement of the rule (tests/junctions_ref.py) -- every event, every tally, the whole span array --, the restatement itself
against what was planted, the writer's text against hand-written lines, the argument errors of `bronko call`, and the four
functions in both engine libraries."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import junction_cases, junctions_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
HPV = os.path.join(ROOT, "tests", "golden", "HPV16.fa")


def _both(ix, g, reads, L=33, M=2):
    """The twin's and the restatement's (rows, span, tallies) of the same reads; asserts that they are equal and returns the latter."""
    rows, span, counters = hostlib.junction_events(ix, 0, reads, L, M)
    res = junctions_ref.junction_events(g, reads, L, M)
    want = junctions_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    assert counters == junctions_ref.counters_tuple(res)
    return res


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = junction_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = junctions_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    cases, text = junction_cases.crafted_cases(k)
    assert text == g.text
    yield k, ix, g, cases
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for L, M in ((33, 2), (33, 0), (1, 2), (32, 8), (401, 4), ((1 << 27) - 1, 2)):
        res = _both(ix, g, reads, L, M)
        assert res.events or L > 1135
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])
        _both(ix, g, [read], 1, 2)


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the junction it supports, or the one tally it adds to."""
    k, ix, g, cases = crafted
    by = {}
    for label, read, expect in cases:
        res = junctions_ref.junction_events(g, [read])
        by[label] = res
        c = res.counters
        against = label.endswith("/rc")
        others = {name: v for name, v in c.items() if v and name not in ("records", "anchored")}
        if expect is None:
            continue
        if expect == "none":
            assert not res.events and not any(res.span) and not others, label
        elif expect == "span":
            assert not res.events and others == {"ref_spanning": 1} and sum(res.span_sums()) >= 1, label
        elif expect in ("short", "backward", "discordant"):
            assert not res.events and not any(res.span) and others == {expect: 1}, label
        else:
            _, cell, d = expect
            assert others == {"supporting": 1} and len(res.events) == 1, (label, res.events, c)
            (pos, dd), (fwd, rev) = next(iter(res.events.items()))
            assert (fwd, rev) == ((0, 1) if against else (1, 0)) and dd == d, label
            assert junction_cases.haplotype(g.text, pos, dd) == junction_cases.haplotype(g.text, cell, d) and pos <= cell, label
            assert g.text[pos - 1] != g.text[pos + d - 1], label    # normalised to the left
    # D = 32 and D = 1 are junctions at min_len 1
    for label, d in (("d32", 32), ("d1", 1)):
        read = next(r for lb, r, _ in cases if lb == label)
        assert [key[1] for key in junctions_ref.junction_events(g, [read], 1, 2).events] == [d]
        assert junctions_ref.junction_events(g, [read], d, 2).events and not junctions_ref.junction_events(g, [read], d + 1, 2).events
    # the shared stretch's first cell, and its length
    first_c = g.first[2]
    for label, (x, y, h) in junction_cases.homology_sites(k).items():
        (pos, d), = by["homology_" + label].events
        assert (pos, d) == (first_c + x, y - x) and junctions_ref.homology(g, pos, d) == h, label
    # one substitution beside the breakpoint moves it; a tie takes the smaller p
    p400 = next(e for lb, _, e in cases if lb == "d400")[1]
    assert list(by["sub_left_of_bp"].events) == [(p400 - 1, 400)] and list(by["tie"].events) == [(p400, 400)]
    if "sub_right_of_bp" in by:
        assert list(by["sub_right_of_bp"].events) == [(p400 + 1, 400)]
    m0 = junctions_ref.junction_events(g, [next(r for lb, r, _ in cases if lb == "tie")], 33, 0)
    assert not m0.events and m0.counters["discordant"] == 1
    for label in ("n_2k", "bp_at_a_plus_k", "bp_at_b", "anchor_try2_front", "anchor_try2_back", "m_eq_M"):
        assert list(by[label].events) == [(p400, 400)], label
    # all of them together: each junction once along and once against the reference, and spanning records at d400's two sides
    res = junctions_ref.junction_events(g, [r for _, r, _ in cases])
    assert all(fwd == rev for fwd, rev in res.events.values())
    row = next(r for r in junctions_ref.table_rows(g, res) if r[:2] == (p400, 400))
    assert row[2] == row[3] >= 6 and row[4] == 2 and row[5] == 2


@pytest.fixture(scope="module")
def hpv_sample():
    g = {k: junctions_ref.read_fasta(HPV, k) for k in (21, 31)}
    reads, planted = junction_cases.sample_reads(g[21].text)
    return g, reads, planted


@pytest.mark.parametrize("k", [21, 31])
def test_sample_twin_equals_restatement(hpv_sample, k):
    g, reads, planted = hpv_sample
    ix = HostIndex.build(k, [HPV])
    try:
        res = _both(ix, g[k], reads)
        assert res.counters["records"] == len(reads)
        _both(ix, g[k], reads[:400], 1, 0)
        _both(ix, g[k], reads[:400], 100, 8)
    finally:
        ix.close()


def test_sample_is_not_vacuous(hpv_sample):
    """The restatement alone finds every planted junction on both strands with spanning records at both of its sides, every tally
    is used, and nothing that was not planted gathers reads."""
    g, reads, planted = hpv_sample
    g = g[21]
    res = junctions_ref.junction_events(g, reads)
    assert all(v > 0 for v in res.counters.values()), res.counters
    assert res.counters["ref_spanning"] > 1000 and res.counters["supporting"] > 50
    sums = res.span_sums()
    want = set()
    for pos, d, af in planted:
        hap = junction_cases.haplotype(g.text, pos, d)
        found = [key for key in res.events if key[1] == d and junction_cases.haplotype(g.text, *key) == hap]
        assert len(found) == 1, (pos, d)
        fwd, rev = res.events[found[0]]
        assert fwd >= 1 and rev >= 1 and sums[found[0][0]] > 0 and sums[found[0][0] + d] > 0, (pos, d, fwd, rev)
        want.add(found[0])
    reported = junctions_ref.table_rows(g, res, 5)
    assert reported and {r[:2] for r in reported} <= want
    assert {r[:2] for r in junctions_ref.table_rows(g, res, 1)} == set(res.events)


def test_writer_text(tmp_path):
    """Hand-written lines: the order is (sequence, donor, acceptor), freq is truncated, homology comes from the reference."""
    k = 21
    seqs = junction_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    try:
        g = junctions_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
        first_b, first_c = g.first[1], g.first[2]
        (x1, y1, _), (x6, y6, _), (xk, yk, _) = (junction_cases.homology_sites(k)[n] for n in ("one", "six", "k_minus_1"))
        rows = [(first_c + xk, yk - xk, 2, 1, 6, 9), (first_c + x6, y6 - x6, 3, 0, 0, 4), (first_c + x1, y1 - x1, 1, 1, 1, 0),
                (first_c + x1, 40, 7, 0, 14, 2), (first_b + 100, 50, 0, 5, 10, 10), (760, 400, 1, 2, 4, 5), (760, 33, 1, 0, 2, 0)]
        path = str(tmp_path / "x.junctions.tsv")
        hostlib.write_junctions_tsv(path, ix, 0, rows, 33, 2, 1)
        text = open(path).read()
        h = {key: junctions_ref.homology(g, *key) for key in [r[:2] for r in rows]}
        assert (h[(first_c + x1, y1 - x1)], h[(first_c + x6, y6 - x6)], h[(first_c + xk, yk - xk)]) == (1, 6, k - 1)
        want = ["##junction_min_len=33", "##junction_max_mismatches=2", "##junction_min_reads=1",
                "chrom\tdonor\tacceptor\tlength\tfwd\trev\treads\tspan_donor\tspan_acceptor\tfreq\thomology",
                "craftA\t760\t794\t33\t1\t0\t1\t2\t0\t0.3333\t%d" % h[(760, 33)],
                "craftA\t760\t1161\t400\t1\t2\t3\t4\t5\t0.4285\t%d" % h[(760, 400)],
                "craftB\t100\t151\t50\t0\t5\t5\t10\t10\t0.3333\t%d" % h[(first_b + 100, 50)],
                "craftC\t%d\t%d\t40\t7\t0\t7\t14\t2\t0.3333\t%d" % (x1, x1 + 41, h[(first_c + x1, 40)]),
                "craftC\t%d\t%d\t%d\t1\t1\t2\t1\t0\t0.6666\t1" % (x1, y1 + 1, y1 - x1),
                "craftC\t%d\t%d\t%d\t3\t0\t3\t0\t4\t1.0000\t6" % (x6, y6 + 1, y6 - x6),
                "craftC\t%d\t%d\t%d\t2\t1\t3\t6\t9\t0.3333\t%d" % (xk, yk + 1, yk - xk, k - 1)]
        assert text == "".join(line + "\n" for line in want)
        assert text == junctions_ref.tsv_text(g, rows, 33, 2, 1)
        # homology stops at the sequence's end: a junction whose acceptor side is craftA's last cells
        end_a = g.first[1]
        hostlib.write_junctions_tsv(path, ix, 0, [(end_a - 50, 47, 1, 0, 0, 0)], 5, 0, 7)
        last = open(path).read().splitlines()
        assert last[:3] == ["##junction_min_len=5", "##junction_max_mismatches=0", "##junction_min_reads=7"]
        assert int(last[-1].split("\t")[-1]) == junctions_ref.homology(g, end_a - 50, 47) <= 3
        hostlib.write_junctions_tsv(path, ix, 0, [], 33, 2, 5)   # a sample without events: the headers alone
        assert open(path).read() == junctions_ref.tsv_text(g, [], 33, 2, 5) and open(path).read().endswith("freq\thomology\n")
        with pytest.raises(RuntimeError):                          # an event that is no junction of one sequence
            hostlib.write_junctions_tsv(path, ix, 0, [(end_a - 10, 40, 1, 0, 0, 0)], 33, 2, 5)
    finally:
        ix.close()
    assert junctions_ref.freq_text(1, 2) == "0.3333" and junctions_ref.freq_text(3, 0) == "1.0000" and junctions_ref.freq_text(2, 1) == "0.6666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--junction-min-len", "50"], "--junctions"), (["--junction-max-mismatches", "1"], "--junctions"),
                        (["--junction-min-reads", "3"], "--junctions"),
                        (["--junctions", "--junction-min-len", "0"], "--junction-min-len"), (["--junctions", "--junction-min-len", "-4"], "--junction-min-len"),
                        (["--junctions", "--junction-min-len", str(1 << 27)], "--junction-min-len"),
                        (["--junctions", "--junction-max-mismatches", "9"], "--junction-max-mismatches"),
                        (["--junctions", "--junction-max-mismatches", "-1"], "--junction-max-mismatches"),
                        (["--junctions", "--junction-min-reads", "0"], "--junction-min-reads")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--junctions")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
    usage = _run("call", "--help")
    for flag in ("--junctions", "--junction-min-len", "--junction-max-mismatches", "--junction-min-reads"):
        assert flag in usage.stdout + usage.stderr, flag


def test_both_libraries_export_the_four_functions():
    names = ("bk_junctions_enable", "bk_sample_junctions", "bk_sample_download_junctions", "bk_sample_download_junction_span")
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        assert L.bk_abi_version() == 8
        for name in names:
            assert hasattr(L, name) and name in _ffi.SYMBOLS, name
    import ctypes as C
    assert C.sizeof(_ffi.JunctionConfig) == 12 and C.sizeof(_ffi.JunctionParams) == 8 and C.sizeof(_ffi.JunctionSummary) == 80
