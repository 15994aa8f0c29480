"""`bronko call --breakends` without a GPU: the host twin (bronko_amd/host/breakends.cpp through bh_breakend_events) against the Python
restatement of the rule (tests/breakends_ref.py) -- every event, every tally, the whole span array --, the restatement itself against
what was planted, a read against its reverse complement, the writer's text against hand-written lines, the argument errors of
`bronko call`, and the four functions in both engine libraries."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import breakend_cases, breakends_ref
from tests.breakends_ref import L, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
SETTINGS = ((20, 2), (16, 0), (40, 8))


def _both(ix, g, reads, C=20, M=2):
    """The twin's and the restatement's (rows, span, tallies) of the same reads; asserts that they are equal and returns the latter."""
    rows, span, counters = hostlib.breakend_events(ix, 0, reads, C, M)
    res = breakends_ref.breakend_events(g, reads, C, M)
    want = breakends_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    assert counters == breakends_ref.counters_tuple(res)
    return res


def _genome(seqs, k):
    return breakends_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = breakend_cases.crafted_genome()
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = _genome(seqs, k)
    cases, text = breakend_cases.crafted_cases(k)
    assert text == g.text
    yield k, ix, g, cases
    ix.close()


def test_crafted_genome(crafted):
    k, ix, g, cases = crafted
    a, b, c = g.seqs
    assert g.names == ["bkA", "bkB", "bkC"] and "N" not in a + c
    assert b[breakend_cases.N_RUN[0]:breakend_cases.N_RUN[1]] == "N" * 20 and b.count("N") == 20
    u, v, h = breakend_cases.REPEAT
    assert c[u:u + h] == c[v:v + h] and h >= k + 24
    lens = {len(r) for _, r, _ in cases}
    assert {64, 150, 300, 2 * k - 1, 2 * k, 159, 160, 161, 255, 256, 257} <= lens and min(lens) == 2 * k - 1


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for C, M in SETTINGS + ((25, 1), (17, 3)):
        res = _both(ix, g, reads, C, M)
        assert res.events
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the site it supports, or the one tally it adds to."""
    k, ix, g, cases = crafted
    by = {}
    one = ("supporting", "short", "through", "discordant", "unplaced")
    for label, read, expect in cases:
        res = breakends_ref.breakend_events(g, [read])
        by[label] = res
        c = res.counters
        assert c["records"] == 1, label
        assert c["one_anchor"] == sum(c[name] for name in one) <= 1 and c["one_anchor"] + c["ref_spanning"] <= 1, (label, c)
        used = {name for name, v in c.items() if v} - {"records", "one_anchor"}
        if expect is None:
            continue
        if expect == "nothing":
            assert not res.events and not any(res.span) and not used and c["one_anchor"] == 0, (label, c)
        elif expect == "span":
            assert not res.events and used == {"ref_spanning"} and sum(res.span_sums()) >= 1, (label, c)
        elif isinstance(expect, str):
            assert not res.events and not any(res.span) and used == {expect} and c["one_anchor"] == 1, (label, c)
        else:
            assert used == {"supporting"} and not any(res.span), (label, c)
            assert [key[:2] for key in res.events] == [expect[1:]], (label, list(res.events), expect)
    fa, fb, fc = g.first
    # a read and its reverse complement: the same event, counted on the opposite strand
    for label, read, expect in cases:
        if not label.endswith("/rc"):
            a, b = by[label], by[label + "/rc"]
            assert list(a.events) == list(b.events) and [v[::-1] for v in a.events.values()] == list(b.events.values()), label
            assert a.span == b.span and a.counters == b.counters, label
            if a.events:
                assert list(a.events.values()) == [[1, 0]], label
    t = g.text
    idx = breakend_cases._idx(t)
    x, y = fa + 400, fa + 800
    # the tie: the tag begins (ends) with the substituted base; the extension: the event is the unbroken read's, the mismatch in m
    (cell, side, tag), = by["L_mismatch_then_4"].events
    assert cell == x - 5 and tag[0] != t[x - 4] and tag[1:5] == t[x - 3:x + 1]
    (cell, side, tag), = by["R_mismatch_then_4"].events
    assert cell == y + 5 and tag[-1] != t[y + 4] and tag[-5:-1] == t[y:y + 4]
    for name in ("L_mismatch_then_5", "R_mismatch_then_5", "L_clip_20", "R_clip_21"):
        read = next(r for lb, r, _ in cases if lb == name)
        assert breakends_ref.breakend_events(g, [read], 20, 0).counters["discordant"] == 1, name
    # clip = C - 1, C, C + 1 and 16: the same four records at C = 16 all support, at C = 22 none does
    for side in "LR":
        for clip in (19, 20, 21, 16):
            read = next(r for lb, r, _ in cases if lb == "%s_clip_%d" % (side, clip))
            assert breakends_ref.breakend_events(g, [read], 16, 2).counters["supporting"] == 1
            assert breakends_ref.breakend_events(g, [read], 22, 2).counters["short"] == 1
    # the walk stops at the border and at the run of N although the next cells match the record
    (cell, side, tag), = by["last_cell_of_b"].events
    assert cell == fc - 1 and tag[:breakend_cases.EDGE] == t[fc:fc + breakend_cases.EDGE]
    (cell, side, tag), = by["first_cell_of_b"].events
    assert cell == fb and tag[-breakend_cases.EDGE:] == t[fb - breakend_cases.EDGE:fb]
    n0, n1 = fb + breakend_cases.N_RUN[0], fb + breakend_cases.N_RUN[1]
    (cell, side, tag), = by["stops_below_n_run"].events
    assert cell == n0 - 1 and tag[:breakend_cases.EDGE] == idx[n0:n0 + breakend_cases.EDGE] == "A" * breakend_cases.EDGE
    (cell, side, tag), = by["stops_above_n_run"].events
    assert cell == n1 and tag[-breakend_cases.EDGE:] == "A" * breakend_cases.EDGE
    # two tags at one cell are two events, one base apart too; the site counts them all
    res = breakends_ref.breakend_events(g, [r for lb, r, _ in cases if lb in ("L_plain", "L_second_tag", "L_tag_one_base_apart", "L_plain/rc")])
    assert len(res.events) == 3 and res.site_reads() == {(x, L): 4}
    rows = breakends_ref.table_rows(g, res)
    assert [r[5] for r in rows] == [4, 4, 4] and sorted(r[3] + r[4] for r in rows) == [1, 1, 2]
    # the anchors at the second to fourth offset: m counts what lies in front of them
    for side in "LR":
        read = next(r for lb, r, _ in cases if lb == side + "_anchor_try4")
        assert breakends_ref.breakend_events(g, [read], 20, 3).counters["supporting"] == 1
        read = next(r for lb, r, _ in cases if lb == side + "_anchor_try3")
        assert breakends_ref.breakend_events(g, [read], 20, 1).counters["discordant"] == 1
        read = next(r for lb, r, _ in cases if lb == side + "_m_eq_M_plus_1")
        assert breakends_ref.breakend_events(g, [read], 20, 3).counters["supporting"] == 1
    # all of them together: every tally, both sides, both strands, both kinds of terminus, a span above zero at an event
    res = breakends_ref.breakend_events(g, [r for _, r, _ in cases])
    assert all(v > 0 for v in res.counters.values()), res.counters
    assert {key[1] for key in res.events} == {L, R} and all(f == r for f, r in res.events.values())
    rows = breakends_ref.table_rows(g, res)
    text = breakends_ref.tsv_text(g, rows, 20, 2, 1, breakends_ref.tallies10(res, 1))
    term = [line.split("\t") for line in text.splitlines()[5:] if line.split("\t")[9] == "1"]
    assert {(f[0], f[2]) for f in term} == {("bkA", "R"), ("bkB", "R"), ("bkB", "L"), ("bkC", "L")} and all(f[7] == "0" for f in term)
    assert any(r[0] == x and r[6] > 0 for r in rows) and any(r[0] == y and r[6] > 0 for r in rows)


@pytest.fixture(scope="module")
def fuzz():
    seqs, reads = breakend_cases.fuzz_world()
    return seqs, reads, {k: _genome(seqs, k) for k in (21, 31)}


def test_fuzz_is_not_vacuous(fuzz):
    """Conditions the restatement meets alone: every tally above zero, both sides on both strands, sites with several tags, events at
    termini, and a read and its reverse complement give the same events."""
    seqs, reads, gs = fuzz
    g = gs[21]
    assert 3 <= len(seqs) <= 5 and any("N" in s for _, s in seqs) and len(reads) == 2000
    res = breakends_ref.breakend_events(g, reads)
    assert all(v > 0 for v in res.counters.values()), res.counters
    assert res.counters["supporting"] >= 300 and len(res.events) >= 100
    for side in (L, R):
        assert sum(f for (c, s, t), (f, r) in res.events.items() if s == side) >= 50
        assert sum(r for (c, s, t), (f, r) in res.events.items() if s == side) >= 50
    tags = {}
    for (c, s, t) in res.events:
        tags[(c, s)] = tags.get((c, s), 0) + 1
    assert sum(1 for v in tags.values() if v >= 2) >= 10
    assert any(f + r >= 5 for f, r in res.events.values())
    rows = breakends_ref.table_rows(g, res)
    assert any(r[6] > 0 for r in rows)
    text = breakends_ref.tsv_text(g, rows, 20, 2, 1, breakends_ref.tallies10(res, 1))
    assert sum(1 for line in text.splitlines()[5:] if line.split("\t")[9] == "1") >= 2
    for r in reads[:300]:
        a, b = breakends_ref.breakend_events(g, [r]), breakends_ref.breakend_events(g, [breakends_ref.revcomp(r)])
        assert list(a.events) == list(b.events) and [v[::-1] for v in a.events.values()] == list(b.events.values())
        assert a.span == b.span and a.counters == b.counters


@pytest.mark.parametrize("k", [21, 31])
def test_fuzz_twin_equals_restatement(fuzz, k):
    seqs, reads, gs = fuzz
    ix = HostIndex.build_mem(k, [("fuzz", [(name, s.encode()) for name, s in seqs])])
    try:
        res = _both(ix, gs[k], reads)
        assert res.counters["records"] >= len(reads) and res.events
        _both(ix, gs[k], reads[:600], 16, 0)
        _both(ix, gs[k], reads[:600], 40, 8)
    finally:
        ix.close()


def test_writer_text(tmp_path):
    """Hand-written lines: the order is (sequence, pos, side with L first, tag by its letters), positions are 1-based within their
    sequence, freq is truncated, terminus marks the first cell held from above and the last held from below."""
    k = 21
    seqs = breakend_cases.crafted_genome()
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    try:
        g = _genome(seqs, k)
        fa, fb, fc = g.first
        code = breakends_ref.seq_code
        ta, tc, tt = "ACGTACGTACGTACGT", "CCGTACGTACGTACGT", "TTTTTTTTTTTTTTTA"
        # rows as bk_breakend_record: (cell, tag, side, fwd, rev, site_reads, span, 0)
        rows = [(fc - 1, code(ta), 0, 2, 1, 3, 0, 0), (fb, code(tt), 1, 1, 0, 1, 0, 0), (fb, code(ta), 0, 1, 1, 2, 4, 0), (100, code(tc), 1, 0, 5, 7, 10, 0),
                (100, code(ta), 1, 1, 1, 7, 10, 0), (100, code(tt), 0, 3, 0, 3, 0, 0), (fc, code(ta), 0, 1, 0, 1, 2, 0)]
        tallies = (100, 30, 60, 17, 4, 3, 2, 4, 9, 7)
        path = str(tmp_path / "x.breakends.tsv")
        hostlib.write_breakends_tsv(path, ix, 0, rows, 20, 2, 1, tallies)
        text = open(path).read()
        want = ["##breakend_min_clip=20", "##breakend_max_mismatches=2", "##breakend_min_reads=1",
                "##breakend_tallies=records:100,one_anchor:30,ref_spanning:60,supporting:17,short:4,through:3,discordant:2,unplaced:4,candidates:9,reported:7",
                "chrom\tpos\tside\tfwd\trev\treads\tsite_reads\tspan\tfreq\tterminus\ttag",
                "bkA\t101\tL\t3\t0\t3\t3\t0\t1.0000\t0\t" + tt,
                "bkA\t101\tR\t1\t1\t2\t7\t10\t0.1666\t0\t" + ta,
                "bkA\t101\tR\t0\t5\t5\t7\t10\t0.3333\t0\t" + tc,
                "bkB\t1\tL\t1\t1\t2\t2\t4\t0.3333\t0\t" + ta,
                "bkB\t1\tR\t1\t0\t1\t1\t0\t1.0000\t1\t" + tt,
                "bkB\t1200\tL\t2\t1\t3\t3\t0\t1.0000\t1\t" + ta,
                "bkC\t1\tL\t1\t0\t1\t1\t2\t0.3333\t0\t" + ta]
        assert text == "".join(line + "\n" for line in want)
        assert text == breakends_ref.tsv_text(g, rows, 20, 2, 1, tallies)
        hostlib.write_breakends_tsv(path, ix, 0, [], 16, 0, 7, (5, 0, 5, 0, 0, 0, 0, 0, 0, 0))     # a sample without events: the five lines
        assert open(path).read() == breakends_ref.tsv_text(g, [], 16, 0, 7, (5, 0, 5, 0, 0, 0, 0, 0, 0, 0)) and len(open(path).read().splitlines()) == 5
        assert open(path).read().splitlines()[:3] == ["##breakend_min_clip=16", "##breakend_max_mismatches=0", "##breakend_min_reads=7"]
        # a cell outside the file, a cell on a letter that is not ACGT, a side above 1
        for bad in ((g.cells, 0, 0, 1, 0, 1, 0, 0), (fb + breakend_cases.N_RUN[0] + 3, 0, 0, 1, 0, 1, 0, 0), (100, 0, 2, 1, 0, 1, 0, 0)):
            with pytest.raises(RuntimeError):
                hostlib.write_breakends_tsv(path, ix, 0, [bad], 20, 2, 5, tallies)
        with pytest.raises(RuntimeError):
            hostlib.breakend_events(ix, 0, ["ACGT"], 15, 2)
        with pytest.raises(RuntimeError):
            hostlib.breakend_events(ix, 0, ["ACGT"], 20, 9)
    finally:
        ix.close()
    f = breakends_ref.freq_text
    assert f(1, 2) == "0.3333" and f(3, 0) == "1.0000" and f(2, 1) == "0.6666" and f(1, 5) == "0.1666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--breakend-min-clip", "30"], "--breakend-min-clip needs --breakends"),
                        (["--breakend-max-mismatches", "1"], "--breakend-max-mismatches needs --breakends"),
                        (["--breakend-min-reads", "3"], "--breakend-min-reads needs --breakends"),
                        (["--breakends", "--breakend-min-clip", "15"], "--breakend-min-clip must be between 16 and 65519, got 15"),
                        (["--breakends", "--breakend-min-clip", "65520"], "--breakend-min-clip must be between 16 and 65519, got 65520"),
                        (["--breakends", "--breakend-max-mismatches", "9"], "--breakend-max-mismatches must be between 0 and 8, got 9"),
                        (["--breakends", "--breakend-max-mismatches", "-1"], "--breakend-max-mismatches must be between 0 and 8, got -1"),
                        (["--breakends", "--breakend-min-reads", "0"], "--breakend-min-reads must be at least 1, got 0")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    for flag in ("--breakend-min-clip", "--breakend-max-mismatches", "--breakend-min-reads"):
        r = _run(*base, "--breakends", flag, "x")
        assert r.returncode == 2 and "invalid value 'x' for '%s'" % flag in r.stderr
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--breakends")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
    usage = _run("call", "--help")
    for flag in ("--breakends", "--breakend-min-clip", "--breakend-max-mismatches", "--breakend-min-reads", ".breakends.tsv"):
        assert flag in usage.stdout + usage.stderr, flag


def test_both_libraries_export_the_four_functions():
    names = ("bk_breakends_enable", "bk_sample_breakends", "bk_sample_download_breakends", "bk_sample_download_breakend_span")
    for testing in (False, True):
        lib = _ffi.load(testing=testing)
        assert lib.bk_abi_version() == 8
        for name in names:
            assert hasattr(lib, name) and name in _ffi.SYMBOLS, name
    import ctypes as C
    assert C.sizeof(_ffi.BreakendConfig) == 12 and C.sizeof(_ffi.BreakendParams) == 8 and C.sizeof(_ffi.BreakendSummary) == 88
