"""`bronko call --copybacks` without a GPU: the host twin (bronko_amd/host/copybacks.cpp through bh_copyback_events) against the
Python restatement of the rule (tests/copybacks_ref.py) -- every event, every tally, the whole span array --, the restatement itself
against what was crafted, the writer's text against hand-written lines, the argument errors of `bronko call`, and the four
functions in both engine libraries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import copyback_cases, copybacks_ref
from tests.copybacks_ref import H, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _both(ix, g, reads, M=2):
    """The twin's and the restatement's (rows, span, tallies) of the same reads; asserts that they are equal and returns the latter."""
    rows, span, counters = hostlib.copyback_events(ix, 0, reads, M)
    res = copybacks_ref.copyback_events(g, reads, M)
    want = copybacks_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    assert counters == copybacks_ref.counters_tuple(res)
    return res


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = copyback_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = copybacks_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    cases, text = copyback_cases.crafted_cases(k)
    assert text == g.text
    yield k, ix, g, cases
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for M in (2, 0, 1, 3, 8):
        assert _both(ix, g, reads, M).events
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the event it supports, or the one tally it adds to."""
    k, ix, g, cases = crafted
    by = {}
    for label, read, expect in cases:
        res = copybacks_ref.copyback_events(g, [read])
        by[label] = res
        others = {name: v for name, v in res.counters.items() if v and name not in ("records", "same_strand", "switched")}
        if expect is None:
            continue
        if expect == "none":
            assert not res.events and not any(res.span) and not others, label
        elif expect == "span":
            assert not res.events and others == {"ref_spanning": 1} and sum(res.span_sums()) >= 1 and res.counters["same_strand"] == 1, label
        elif expect == "discordant":
            assert not res.events and not any(res.span) and others == {"discordant": 1}, label
        else:
            assert others == {"supporting": 1} and res.counters["switched"] == 1 and list(res.events) == [expect[1:]], (label, res.events)
    # a read and its reverse complement: the same event, the other counter (a hairpin's two cells are one: both count lo_first)
    for label, _, expect in cases:
        if label.endswith("/rc") or not by[label].events:
            continue
        (key, (lf, hf)), = by[label].events.items()
        (key2, (lf2, hf2)), = by[label + "/rc"].events.items()
        assert key == key2 and lf + hf == 1, label
        if "hairpin" not in label:
            assert (lf2, hf2) == (hf, lf), label
    assert by["H_hairpin"].events == by["H_hairpin/rc"].events and by["T_hairpin"].events == by["T_hairpin/rc"].events
    (_, lo, hi), = by["H_hairpin"].events
    assert lo == hi
    # each palindrome length is the event's homology; the hairpin in the palindrome crosses x = y over all of it
    first_d = g.first[3]
    for kind, name in ((H, "H"), (T, "T")):
        for label, (u, v, h) in copyback_cases.turn_sites(k).items():
            (key,) = by["%s_palindrome_%s" % (name, label)].events
            assert copybacks_ref.homology(g, *key) == h, (name, label)
        (key,) = by[name + "_hairpin_palindrome"].events
        assert by[name + "_hairpin_palindrome_off_centre"].events.keys() == {key} and copybacks_ref.homology(g, *key) == copyback_cases.HAIRPIN[1]
        (key,) = by[name + "_plain"].events
        assert copybacks_ref.homology(g, *key) == 0 and key[1] >= first_d
        # one substitution more than M is discordant at M, supporting at M + 1
        read = next(r for lb, r, _ in cases if lb == name + "_m_eq_M_plus_1")
        assert copybacks_ref.copyback_events(g, [read], 3).events.keys() == {key}
        read = next(r for lb, r, _ in cases if lb == name + "_m_eq_M")
        assert copybacks_ref.copyback_events(g, [read], 1).counters["discordant"] == 1
        for label in ("_bp_at_f_plus_k", "_bp_at_g", "_n_2k", "_n_64", "_anchor_try2_front", "_anchor_try2_back", "_m_eq_M"):
            assert by[name + label].events.keys() == {key}, name + label
    # all of them together: every event of a non-hairpin pair met from either cell equally often
    res = copybacks_ref.copyback_events(g, [r for _, r, _ in cases])
    assert all(lf == hf for (_, lo, hi), (lf, hf) in res.events.items() if lo != hi and hi - lo != copyback_cases.HAIRPIN[1])
    assert {key[0] for key in res.events} == {H, T}


@pytest.fixture(scope="module")
def fuzz():
    seqs, reads = copyback_cases.fuzz_world()
    return seqs, reads, copybacks_ref.Genome([n for n, _ in seqs], [s for _, s in seqs], 21)


def test_fuzz_is_not_vacuous(fuzz):
    """The restatement alone: at least 200 supporting records of each kind, at least 20 events with homology, every tally used, and
    a read and its reverse complement give the same event."""
    seqs, reads, g = fuzz
    res = copybacks_ref.copyback_events(g, reads)
    assert all(v > 0 for v in res.counters.values()), res.counters
    for kind in (H, T):
        assert sum(lf + hf for key, (lf, hf) in res.events.items() if key[0] == kind) >= 200
    assert sum(1 for key in res.events if copybacks_ref.homology(g, *key) > 0) >= 20
    assert any(lo == hi for _, lo, hi in res.events)
    for r in reads[:300]:
        assert copybacks_ref.copyback_events(g, [r]).events.keys() == copybacks_ref.copyback_events(g, [copybacks_ref.revcomp(r)]).events.keys()


@pytest.mark.parametrize("k", [21, 31])
def test_fuzz_twin_equals_restatement(fuzz, k):
    seqs, reads, _ = fuzz
    g = copybacks_ref.Genome([n for n, _ in seqs], [s for _, s in seqs], k)
    ix = HostIndex.build_mem(k, [("fuzz", [(name, s.encode()) for name, s in seqs])])
    try:
        res = _both(ix, g, reads)
        assert res.counters["records"] == len(reads) and res.events
        _both(ix, g, reads[:500], 0)
        _both(ix, g, reads[:500], 8)
    finally:
        ix.close()


def test_writer_text(tmp_path):
    """Hand-written lines: the order is (sequence, kind, lo, hi), cells are 1-based, freq is truncated over the larger span,
    homology comes from the reference."""
    k = 21
    seqs = copyback_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    try:
        g = copybacks_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
        first_b, first_d = g.first[1], g.first[3]
        (u1, v1, _), (u6, v6, _), (uk, vk, _) = (copyback_cases.turn_sites(k)[n] for n in ("one", "six", "k_minus_1"))
        c, w = copyback_cases.HAIRPIN
        rows = [(first_d + uk, first_d + vk + 1, T, 2, 1, 6, 9, 0), (first_d + u6 - 1, first_d + v6, H, 3, 0, 0, 4, 0),
                (first_d + u1 - 1, first_d + v1, H, 1, 1, 1, 0, 0), (first_d + c - 1, first_d + c + w - 1, H, 7, 0, 14, 2, 0),
                (first_b + 100, first_b + 100, T, 0, 5, 10, 10, 0), (760, 1160, T, 1, 2, 4, 5, 0), (760, 1160, H, 1, 0, 2, 0, 0)]
        path = str(tmp_path / "x.copybacks.tsv")
        hostlib.write_copybacks_tsv(path, ix, 0, rows, 2, 1, 0)
        text = open(path).read()
        h = {r[:3]: copybacks_ref.homology(g, r[2], r[0], r[1]) for r in rows}
        assert [h[r[:3]] for r in rows[:4]] == [k - 1, 6, 1, w]
        want = ["##copyback_max_mismatches=2", "##copyback_min_reads=1", "##copyback_min_dist=0",
                "chrom\tkind\tlo\thi\tdistance\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology",
                "craftA\tH\t761\t1161\t400\t1\t0\t1\t2\t0\t0.3333\t%d" % h[(760, 1160, H)],
                "craftA\tT\t761\t1161\t400\t1\t2\t3\t4\t5\t0.3750\t%d" % h[(760, 1160, T)],
                "craftB\tT\t101\t101\t0\t0\t5\t5\t10\t10\t0.3333\t%d" % h[(first_b + 100, first_b + 100, T)],
                "craftD\tH\t%d\t%d\t%d\t1\t1\t2\t1\t0\t0.6666\t1" % (u1, v1 + 1, v1 - u1 + 1),
                "craftD\tH\t%d\t%d\t%d\t3\t0\t3\t0\t4\t0.4285\t6" % (u6, v6 + 1, v6 - u6 + 1),
                "craftD\tH\t%d\t%d\t%d\t7\t0\t7\t14\t2\t0.3333\t%d" % (c, c + w, w, w),
                "craftD\tT\t%d\t%d\t%d\t2\t1\t3\t6\t9\t0.2500\t%d" % (uk + 1, vk + 2, vk + 1 - uk, k - 1)]
        assert text == "".join(line + "\n" for line in want)
        assert text == copybacks_ref.tsv_text(g, rows, 2, 1, 0)
        hostlib.write_copybacks_tsv(path, ix, 0, [], 0, 7, 30)     # a sample without events: the headers alone
        assert open(path).read() == copybacks_ref.tsv_text(g, [], 0, 7, 30) and open(path).read().endswith("freq\thomology\n")
        assert open(path).read().splitlines()[:3] == ["##copyback_max_mismatches=0", "##copyback_min_reads=7", "##copyback_min_dist=30"]
        for bad in ((first_b - 10, first_b + 10, H, 1, 0, 0, 0, 0), (10, 5, H, 1, 0, 0, 0, 0), (10, 20, 2, 1, 0, 0, 0, 0)):
            with pytest.raises(RuntimeError):                      # cells in two sequences, hi below lo, no such kind
                hostlib.write_copybacks_tsv(path, ix, 0, [bad], 2, 5, 0)
    finally:
        ix.close()
    assert copybacks_ref.freq_text(1, 2, 0) == "0.3333" and copybacks_ref.freq_text(3, 0, 0) == "1.0000" and copybacks_ref.freq_text(2, 0, 1) == "0.6666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--copyback-max-mismatches", "1"], "--copybacks"), (["--copyback-min-reads", "3"], "--copybacks"),
                        (["--copyback-min-dist", "10"], "--copybacks"),
                        (["--copybacks", "--copyback-max-mismatches", "9"], "--copyback-max-mismatches"),
                        (["--copybacks", "--copyback-max-mismatches", "-1"], "--copyback-max-mismatches"),
                        (["--copybacks", "--copyback-min-reads", "0"], "--copyback-min-reads"),
                        (["--copybacks", "--copyback-min-dist", "-1"], "--copyback-min-dist"),
                        (["--copybacks", "--copyback-min-dist", str(1 << 32)], "--copyback-min-dist")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--copybacks")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
    usage = _run("call", "--help")
    for flag in ("--copybacks", "--copyback-max-mismatches", "--copyback-min-reads", "--copyback-min-dist"):
        assert flag in usage.stdout + usage.stderr, flag


def test_both_libraries_export_the_four_functions():
    names = ("bk_copybacks_enable", "bk_sample_copybacks", "bk_sample_download_copybacks", "bk_sample_download_copyback_span")
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        assert L.bk_abi_version() == 8
        for name in names:
            assert hasattr(L, name) and name in _ffi.SYMBOLS, name
    assert C.sizeof(_ffi.CopybackConfig) == 8 and C.sizeof(_ffi.CopybackParams) == 16 and C.sizeof(_ffi.CopybackSummary) == 72
    assert np.zeros((1, 8), np.uint32).nbytes == 32                # bk_copyback_record as the bindings carry it
