"""`bronko call --duplications` without a GPU: the host twin (bronko_amd/host/duplications.cpp through bh_duplication_events) against
the Python restatement of the rule (tests/duplications_ref.py) -- every event, every tally, the whole span array --, the restatement
itself against what was planted, the writer's text against hand-written lines, the argument errors of `bronko call`, and the four
functions in both engine libraries."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import duplication_cases, duplications_ref, indels_ref, junction_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
HPV = os.path.join(ROOT, "tests", "golden", "HPV16.fa")


def _both(ix, g, reads, L=33, M=2):
    """The twin's and the restatement's (rows, span, tallies) of the same reads; asserts that they are equal and returns the latter."""
    rows, span, counters = hostlib.duplication_events(ix, 0, reads, L, M)
    res = duplications_ref.duplication_events(g, reads, L, M)
    want = duplications_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    assert counters == duplications_ref.counters_tuple(res)
    return res


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = duplication_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = duplications_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    cases, text = duplication_cases.crafted_cases(k)
    assert text == g.text
    yield k, ix, g, cases
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for L, M in ((33, 2), (33, 0), (1, 2), (32, 8), (201, 4), ((1 << 27) - 1, 2)):
        res = _both(ix, g, reads, L, M)
        assert res.events or L > 1000
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])
        _both(ix, g, [read], 1, 2)


def _floors(g, pos, e):
    s, lo, hi = duplications_ref.bounds(g, pos, e)
    return duplications_ref._stretch_floor(g, lo, pos - 1), duplications_ref._stretch_floor(g, lo, pos - e)


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the event it supports, or the one tally it adds to."""
    k, ix, g, cases = crafted
    by = {}
    for label, read, expect in cases:
        res = duplications_ref.duplication_events(g, [read])
        by[label] = res
        c = res.counters
        against = label.endswith("/rc")
        others = {name: v for name, v in c.items() if v and name not in ("records", "anchored")}
        if expect is None:
            continue
        if expect == "none":
            assert not res.events and not any(res.span) and not others and c["records"] == 1, (label, c)
            assert c["anchored"] == (0 if label.startswith("n_2k_minus_1") else 1), label
        elif expect == "span":
            assert not res.events and others == {"ref_spanning": 1} and sum(res.span_sums()) >= 1, label
        elif expect in ("short", "forward", "discordant"):
            assert not res.events and not any(res.span) and others == {expect: 1}, (label, c)
        else:
            _, cell, e = expect
            assert others == {"supporting": 1} and len(res.events) == 1, (label, res.events, c)
            (pos, ee), (fwd, rev) = next(iter(res.events.items()))
            assert (fwd, rev) == ((0, 1) if against else (1, 0)) and ee == e, label
            assert duplication_cases.haplotype(g.text, pos, ee) == duplication_cases.haplotype(g.text, cell, e) and pos <= cell, label
            fl, fr = _floors(g, pos, e)                            # normalised to the left: a floor or a letter stops it
            assert pos - 1 == fl or pos - e - 1 < fr or g.text[pos - 1] != g.text[pos - e - 1], label
    first = g.first
    end = [f + len(s) for f, s in zip(g.first, g.seqs)]
    hf = duplication_cases.half(k)
    # the origin reads: one event (hi, hi - lo) each, at the second and at the last sequence, whose end is the end of all cells
    for label, s in (("origin_b", 1), ("origin_d", 3), ("origin_b_150", 1), ("origin_b_sub", 1)):
        assert list(by[label].events) == list(by[label + "/rc"].events) == [(end[s], end[s] - first[s])], label
    assert end[3] == g.cells
    rows = duplications_ref.table_rows(g, by["origin_d"])
    assert duplications_ref.tsv_text(g, rows, 33, 2, 1).splitlines()[-1].split("\t")[:4] == ["craftD", "1", str(len(g.seqs[3])), str(len(g.seqs[3]))]
    assert duplications_ref.tsv_text(g, rows, 33, 2, 1).endswith("\t1\n")
    # which of p0, p1 the sequence clips: p0 = max(a + k, lo - dR), p1 = min(b, hi - dL) with a = 0, b = n - k
    n = duplication_cases.N_LEN

    def clipped(label, left, nn=n):
        _, cell, e = next(x for lb, _, x in cases if lb == label)  # the breakpoint as planted: its offset in the read is `left`
        s, lo, hi = duplications_ref.bounds(g, cell, e)
        dl = cell - left
        dr = dl - e
        return lo - dr > k, hi - dl < nn - k

    assert clipped("origin_b", hf, 2 * hf) == (True, True) and clipped("origin_b_150", 70) == (True, True)
    assert clipped("starts_at_first_cell", 75) == (True, False) and clipped("no_overhang_front", 78) == (True, False)
    assert clipped("ends_at_last_cell", 75) == (False, True)
    assert clipped("e200", 75) == (False, False)
    # the floors: F_R at a sequence's first cell and behind a run of N although the letter in front would let the event slide;
    # F_L behind a run of N
    (pos, e), = by["starts_at_first_cell"].events
    assert pos - e == first[1] and g.text[pos - 1] == g.text[pos - e - 1]
    (pos, e), = by["floor_right_at_n"].events
    assert pos - e == 1320 and g.text[pos - 1] == "A" and g.text[pos - e - 1] == "N"
    (pos, e), = by["floor_left_at_n"].events
    assert (pos, e) == (first[3] + duplication_cases.ND[1] + 1, 300) and _floors(g, pos, e)[0] == pos - 1
    assert duplications_ref.homology(g, pos, e) == k - 1
    # by a letter: the shared stretch's first cell in the second copy, and its length
    for label, (x, y, h) in junction_cases.homology_sites(k).items():
        (pos, e), = by["homology_" + label].events
        assert (pos, e) == (first[2] + y, y - x) and duplications_ref.homology(g, pos, e) == h, label
    # one substitution beside the breakpoint moves it; M and M + 1 substitutions
    p200 = next(x for lb, _, x in cases if lb == "e200")[1]
    (pos, e), = by["sub_left_of_bp"].events                        # (one cell to the left as planted; a letter may let it slide on)
    assert pos <= p200 - 1 and e == 200 and list(by["e200"].events) == [(p200, 200)]
    for label in ("n_2k", "bp_at_a_plus_k", "bp_at_b", "anchor_try2_front", "anchor_try2_back", "m_eq_M"):
        assert list(by[label].events) == [(p200, 200)], label
    m0 = duplications_ref.duplication_events(g, [next(r for lb, r, _ in cases if lb == "m_eq_M")], 33, 1)
    assert not m0.events and m0.counters["discordant"] == 1
    assert duplications_ref.duplication_events(g, [next(r for lb, r, _ in cases if lb == "m_eq_M_plus_1")], 33, 3).events
    # E = 32, 17 and 1 are events at min_len 1, and each at its own length but not one above
    for label, e in (("e32", 32), ("e17", 17), ("e1", 1)):
        read = next(r for lb, r, _ in cases if lb == label)
        assert [key[1] for key in duplications_ref.duplication_events(g, [read], 1, 2).events] == [e]
        assert duplications_ref.duplication_events(g, [read], e, 2).events and not duplications_ref.duplication_events(g, [read], e + 1, 2).events
    # all of them together: each event once along and once against the reference
    res = duplications_ref.duplication_events(g, [r for _, r, _ in cases])
    assert all(fwd == rev for fwd, rev in res.events.values()) and all(v > 0 for v in res.counters.values())


def test_short_duplications_are_the_indel_rules_insertions(crafted):
    """A duplication of E <= 32 bases that lies whole inside the read is an insertion to --indels: of the same length, in front of
    the first duplicated cell, the inserted bases the duplicated ones."""
    k, ix, g, cases = crafted
    for label, e in (("e32", 32), ("e17", 17), ("e1", 1)):
        for suffix in ("", "/rc"):
            read = next(r for lb, r, _ in cases if lb == label + suffix)
            (pos, ee), = duplications_ref.duplication_events(g, [read], 1, 2).events
            (cell, kind, length, s), = indels_ref.indel_events(g, [read], 32, 2).events
            assert (kind, length, cell, s) == (indels_ref.INS, e, pos - ee, g.text[pos - ee:pos]), (label, suffix)


@pytest.fixture(scope="module")
def hpv_sample():
    g = {k: duplications_ref.read_fasta(HPV, k) for k in (21, 31)}
    reads, frequent = duplication_cases.sample_reads(g[21].text)
    return g, reads, frequent


@pytest.mark.parametrize("k", [21, 31])
def test_sample_twin_equals_restatement(hpv_sample, k):
    g, reads, frequent = hpv_sample
    ix = HostIndex.build(k, [HPV])
    try:
        res = _both(ix, g[k], reads)
        assert res.counters["records"] == len(reads)
        _both(ix, g[k], reads[:400], 1, 0)
        _both(ix, g[k], reads[:400], 100, 8)
    finally:
        ix.close()


def test_sample_is_not_vacuous(hpv_sample):
    """The restatement alone finds every frequent duplication on both strands with spanning records at both of its ends and the
    origin as one event of the sequence's length; every tally is used; at least 30 distinct events."""
    g, reads, frequent = hpv_sample
    g = g[21]
    res = duplications_ref.duplication_events(g, reads)
    assert all(v > 0 for v in res.counters.values()), res.counters
    assert res.counters["ref_spanning"] > 500 and res.counters["supporting"] > 300 and len(res.events) >= 30
    sums = res.span_sums()
    want = set()
    for pos, e in frequent:
        hap = duplication_cases.haplotype(g.text, pos, e)
        found = [key for key in res.events if key[1] == e and duplication_cases.haplotype(g.text, *key) == hap]
        assert len(found) == 1, (pos, e)
        fwd, rev = res.events[found[0]]
        assert fwd >= 5 and rev >= 5 and sums[found[0][0]] > 0 and sums[found[0][0] - e] > 0, (pos, e, fwd, rev)
        want.add(found[0])
    origin = (g.cells, g.cells)
    assert res.events[origin][0] >= 5 and res.events[origin][1] >= 5 and sums[0] == sums[g.cells] == 0
    reported = duplications_ref.table_rows(g, res, 10)
    assert {r[:2] for r in reported} == want | {origin}
    assert {r[:2] for r in duplications_ref.table_rows(g, res, 1)} == set(res.events)
    text = duplications_ref.tsv_text(g, reported, 33, 2, 10).splitlines()
    assert len(text) == 9 and [ln.split("\t")[-1] for ln in text[4:]] == ["1", "0", "0", "0", "0"]
    assert text[4].split("\t")[1:4] == ["1", str(g.cells), str(g.cells)]   # the origin sorts first: start 1


def test_writer_text(tmp_path):
    """Hand-written lines: the order is (sequence, start, end), freq is truncated and takes the larger span, homology and whole come
    from the reference."""
    k = 21
    seqs = duplication_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    try:
        g = duplications_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
        first_b, first_c, first_d = g.first[1], g.first[2], g.first[3]
        len_b, len_d = len(g.seqs[1]), len(g.seqs[3])
        (x1, y1, _), (x6, y6, _), (xk, yk, _) = (junction_cases.homology_sites(k)[n] for n in ("one", "six", "k_minus_1"))
        rows = [(first_c + yk, yk - xk, 2, 1, 6, 9), (first_c + y6, y6 - x6, 3, 0, 0, 4), (first_c + y1, y1 - x1, 1, 1, 1, 0),
                (first_d + len_d, len_d, 7, 0, 14, 2), (first_b + len_b, len_b, 0, 5, 10, 10), (first_b + len_b, 50, 1, 1, 0, 0),
                (800, 400, 1, 2, 4, 5), (800, 33, 1, 0, 0, 2)]
        path = str(tmp_path / "x.duplications.tsv")
        hostlib.write_duplications_tsv(path, ix, 0, rows, 33, 2, 1)
        text = open(path).read()
        h = {key: duplications_ref.homology(g, *key) for key in [r[:2] for r in rows]}
        assert (h[(first_c + y1, y1 - x1)], h[(first_c + y6, y6 - x6)], h[(first_c + yk, yk - xk)]) == (1, 6, k - 1)
        assert h[(first_b + len_b, len_b)] == h[(first_d + len_d, len_d)] == h[(first_b + len_b, 50)] == 0   # nothing behind the last cell
        want = ["##duplication_min_len=33", "##duplication_max_mismatches=2", "##duplication_min_reads=1",
                "chrom\tstart\tend\tlength\tfwd\trev\treads\tspan_start\tspan_end\tfreq\thomology\twhole",
                "craftA\t401\t800\t400\t1\t2\t3\t4\t5\t0.3750\t%d\t0" % h[(800, 400)],
                "craftA\t768\t800\t33\t1\t0\t1\t0\t2\t0.3333\t%d\t0" % h[(800, 33)],
                "craftB\t1\t%d\t%d\t0\t5\t5\t10\t10\t0.3333\t0\t1" % (len_b, len_b),
                "craftB\t%d\t%d\t50\t1\t1\t2\t0\t0\t1.0000\t0\t0" % (len_b - 49, len_b),
                "craftC\t%d\t%d\t%d\t1\t1\t2\t1\t0\t0.6666\t1\t0" % (x1 + 1, y1, y1 - x1),
                "craftC\t%d\t%d\t%d\t3\t0\t3\t0\t4\t0.4285\t6\t0" % (x6 + 1, y6, y6 - x6),
                "craftC\t%d\t%d\t%d\t2\t1\t3\t6\t9\t0.2500\t%d\t0" % (xk + 1, yk, yk - xk, k - 1),
                "craftD\t1\t%d\t%d\t7\t0\t7\t14\t2\t0.3333\t0\t1" % (len_d, len_d)]
        assert text == "".join(line + "\n" for line in want)
        assert text == duplications_ref.tsv_text(g, rows, 33, 2, 1)
        hostlib.write_duplications_tsv(path, ix, 0, [(900, 47, 1, 0, 0, 0)], 5, 0, 7)
        last = open(path).read().splitlines()
        assert last[:3] == ["##duplication_min_len=5", "##duplication_max_mismatches=0", "##duplication_min_reads=7"]
        hostlib.write_duplications_tsv(path, ix, 0, [], 33, 2, 5)   # a sample without events: the headers alone
        assert open(path).read() == duplications_ref.tsv_text(g, [], 33, 2, 5) and open(path).read().endswith("homology\twhole\n")
        for bad in ((first_b + 10, 40, 1, 0, 0, 0), (first_b + len_b + 1, 40, 1, 0, 0, 0), (first_b, 0, 1, 0, 0, 0)):   # no event of one sequence
            with pytest.raises(RuntimeError):
                hostlib.write_duplications_tsv(path, ix, 0, [bad], 33, 2, 5)
    finally:
        ix.close()
    f = duplications_ref.freq_text
    assert f(1, 2, 0) == "0.3333" and f(1, 0, 2) == "0.3333" and f(3, 0, 0) == "1.0000" and f(2, 1, 1) == "0.6666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--duplication-min-len", "50"], "--duplication-min-len needs --duplications"),
                        (["--duplication-max-mismatches", "1"], "--duplication-max-mismatches needs --duplications"),
                        (["--duplication-min-reads", "3"], "--duplication-min-reads needs --duplications"),
                        (["--duplications", "--duplication-min-len", "0"], "--duplication-min-len must be between 1 and 134217727, got 0"),
                        (["--duplications", "--duplication-min-len", "-4"], "--duplication-min-len must be between 1 and 134217727, got -4"),
                        (["--duplications", "--duplication-min-len", str(1 << 27)], "--duplication-min-len must be between 1 and 134217727, got 134217728"),
                        (["--duplications", "--duplication-max-mismatches", "9"], "--duplication-max-mismatches must be between 0 and 8, got 9"),
                        (["--duplications", "--duplication-max-mismatches", "-1"], "--duplication-max-mismatches must be between 0 and 8, got -1"),
                        (["--duplications", "--duplication-min-reads", "0"], "--duplication-min-reads must be at least 1, got 0")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    r = _run(*base, "--duplications", "--duplication-min-len", "x")
    assert r.returncode == 2 and "invalid value 'x' for '--duplication-min-len'" in r.stderr
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--duplications")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
    usage = _run("call", "--help")
    for flag in ("--duplications", "--duplication-min-len", "--duplication-max-mismatches", "--duplication-min-reads", ".duplications.tsv"):
        assert flag in usage.stdout + usage.stderr, flag


def test_both_libraries_export_the_four_functions():
    names = ("bk_duplications_enable", "bk_sample_duplications", "bk_sample_download_duplications", "bk_sample_download_duplication_span")
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        assert L.bk_abi_version() == 8
        for name in names:
            assert hasattr(L, name) and name in _ffi.SYMBOLS, name
    import ctypes as C
    assert C.sizeof(_ffi.DuplicationConfig) == 12 and C.sizeof(_ffi.DuplicationParams) == 8 and C.sizeof(_ffi.DuplicationSummary) == 80
