"""`bronko call --chimeras` without a GPU: the host twin (bronko_amd/host/chimeras.cpp through bh_chimera_events) against the Python
restatement of the rule (tests/chimeras_ref.py) -- every event, every tally, the whole span array --, the restatement itself against
what was planted, a read against its reverse complement, the writer's text against hand-written lines, the argument errors of
`bronko call`, and the four functions in both engine libraries."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import chimera_cases, chimeras_ref
from tests.chimeras_ref import L, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _both(ix, g, reads, M=2):
    """The twin's and the restatement's (rows, span, tallies) of the same reads; asserts that they are equal and returns the latter."""
    rows, span, counters = hostlib.chimera_events(ix, 0, reads, M)
    res = chimeras_ref.chimera_events(g, reads, M)
    want = chimeras_ref.table_rows(g, res)
    assert rows == want, ("events", [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), ("span", np.flatnonzero(span != sums)[:5])
    assert counters == chimeras_ref.counters_tuple(res)
    return res


def _genome(seqs, k):
    return chimeras_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = chimera_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = _genome(seqs, k)
    cases, text = chimera_cases.crafted_cases(k)
    assert text == g.text
    yield k, ix, g, cases
    ix.close()


def test_crafted_genome_keeps_the_duplication_tests_cells(crafted):
    from tests import duplication_cases
    k, ix, g, cases = crafted
    base = duplication_cases.crafted_genome(k)
    assert [(n, s) for n, s in zip(g.names[:4], g.seqs[:4])] == [(n.split()[0], s.upper()) for n, s in base] and g.names[4:] == ["craftE", "craftF"]
    e, f = g.seqs[4], g.seqs[5]
    assert e[chimera_cases.E_N_RUN[0]:chimera_cases.E_N_RUN[1]] == "N" * 20 and "N" not in f and len(e) == len(f) == 1200
    for (u, v, h) in chimera_cases.along_sites(k).values():       # copies of exactly h bases: the letters on either side differ
        assert f[v:v + h] == e[u:u + h] and f[v - 1] != e[u - 1] and f[v + h] != e[u + h]
    for (u, v, h) in chimera_cases.turned_sites(k).values():
        assert f[v - h + 1:v + 1] == chimeras_ref.revcomp(e[u:u + h])
        assert chimeras_ref.revcomp(f[v + 1]) != e[u - 1] and chimeras_ref.revcomp(f[v - h]) != e[u + h]
    assert sorted(h for _, _, h in chimera_cases.along_sites(k).values()) == sorted(h for _, _, h in chimera_cases.turned_sites(k).values()) == [1, 6, k - 1]


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, cases = crafted
    reads = [r for _, r, _ in cases]
    for M in (2, 0, 1, 3, 8):
        res = _both(ix, g, reads, M)
        assert res.events
    for label, read, _ in cases:                                   # ... and one by one, so that a difference names its record
        _both(ix, g, [read])


def test_crafted_records_are_what_they_are_meant_to_be(crafted):
    """The restatement on each crafted record alone: the event it supports, or the one tally it adds to."""
    k, ix, g, cases = crafted
    by = {}
    for label, read, expect in cases:
        res = chimeras_ref.chimera_events(g, [read])
        by[label] = res
        c = res.counters
        others = {name: v for name, v in c.items() if v and name not in ("records", "crossed", "same_strand")}
        assert c["records"] == 1, label
        if expect is None:
            continue
        if expect == "nothing":
            assert not res.events and not any(res.span) and {name for name, v in c.items() if v} == {"records"}, (label, c)
        elif expect == "none":
            assert not res.events and not any(res.span) and not others and c["crossed"] + c["same_strand"] == 1, (label, c)
        elif expect == "span":
            assert not res.events and others == {"ref_spanning": 1} and c["same_strand"] == 1 and c["crossed"] == 0 and sum(res.span_sums()) >= 1, label
        elif expect == "discordant":
            assert not res.events and not any(res.span) and others == {"discordant": 1} and c["crossed"] == 1, (label, c)
        else:
            assert others == {"supporting": 1} and c["crossed"] == 1 and c["same_strand"] == 0 and not any(res.span), (label, c)
            assert list(res.events) == [expect[1:]], (label, list(res.events), expect)
            lo, s_lo, hi, s_hi = expect[1:]
            assert lo < hi and g.seq_of(lo) != g.seq_of(hi), label
    fa, fb, fc, fd, fe, ff = g.first
    # a read and its reverse complement: the same key, counted on opposite sides
    for label, read, expect in cases:
        if not label.endswith("/rc"):
            a, b = by[label], by[label + "/rc"]
            assert list(a.events) == list(b.events) and [v[::-1] for v in a.events.values()] == list(b.events.values()), label
            assert a.span == b.span and a.counters == b.counters, label
    assert by["LR_e_then_f"].events[next(iter(by["LR_e_then_f"].events))] == [1, 0]      # arm A lies at lo: craftE's cell
    assert by["LR_f_then_e"].events[next(iter(by["LR_f_then_e"].events))] == [0, 1]
    # the same two cells with all four side combinations: four events
    keys = [next(iter(by[name + "_e_then_f"].events)) for name, _, _ in chimera_cases.ORIENTATIONS]
    assert len(set(keys)) == 4 and len({(key[0], key[2]) for key in keys}) == 1 and {(key[1], key[3]) for key in keys} == {(L, R), (L, L), (R, R), (R, L)}
    # the homology of every planted stretch in every orientation class, and none at the free pairs
    for cls in ("LR", "RL", "LL", "RR", "LR_homology_f_then_e"):
        for label, h in (("one", 1), ("six", 6), ("k_minus_1", k - 1)):
            name = "%s_%s" % (cls, label) if cls.endswith("then_e") else "%s_homology_%s" % (cls, label)
            (key,) = by[name].events
            assert chimeras_ref.homology(g, *key) == h, (name, key)
    assert all(chimeras_ref.homology(g, *key) == 0 for key in keys)
    # the slides that a border stops: the letters alone would go on
    t = g.text
    (lo, s_lo, hi, s_hi), = by["slide_stops_at_first_cell"].events
    assert lo == fe and t[hi] == t[lo - 1] and chimeras_ref.homology(g, lo, s_lo, hi, s_hi) == chimera_cases.EDGE
    (lo, s_lo, hi, s_hi), = by["slide_stops_at_last_cell"].events
    assert lo + chimera_cases.EDGE == ff - 1 and t[ff] == t[hi + chimera_cases.EDGE] and chimeras_ref.homology(g, lo, s_lo, hi, s_hi) == chimera_cases.EDGE
    (lo, s_lo, hi, s_hi), = by["slide_stops_at_n_run"].events
    assert t[lo - 1] == "N" and t[hi] == "A" and chimeras_ref.homology(g, lo, s_lo, hi, s_hi) == chimera_cases.EDGE
    # neighbours in the index on one strand: delta = 0 in cell arithmetic, crossed all the same
    for label in ("last_of_e_first_of_f", "last_of_d_first_of_e", "last_of_a_first_of_b_try2"):
        (lo, s_lo, hi, s_hi), = by[label].events
        assert hi == lo + 1 and (s_lo, s_hi) == (L, R) and by[label].counters["ref_spanning"] == 0, label
    # M and M + 1 substitutions
    for name, _, _ in chimera_cases.ORIENTATIONS:
        read = next(r for lb, r, _ in cases if lb == name + "_m_eq_M")
        assert chimeras_ref.chimera_events(g, [read], 1).counters["discordant"] == 1
        read = next(r for lb, r, _ in cases if lb == name + "_m_eq_M_plus_1")
        assert list(chimeras_ref.chimera_events(g, [read], 3).events) == [keys[[o[0] for o in chimera_cases.ORIENTATIONS].index(name)]]
    # all of them together: each event once from either cell, every tally used
    res = chimeras_ref.chimera_events(g, [r for _, r, _ in cases])
    assert all(lf == hf for lf, hf in res.events.values()) and all(v > 0 for v in res.counters.values())
    assert min(len(r) for _, r, _ in cases) == 2 * k - 1 and {64, 150, 2 * k} <= {len(r) for _, r, _ in cases}


@pytest.fixture(scope="module")
def fuzz():
    seqs, reads = chimera_cases.fuzz_world()
    return seqs, reads, {k: _genome(seqs, k) for k in (21, 31)}


def _orientation(g, rec):
    """(s_f, s_g) of a record's two end anchors"""
    k, n = g.k, len(rec)
    front = chimeras_ref._end_anchor(g, rec, [0, 8, 16, 24])
    back = chimeras_ref._end_anchor(g, rec, [n - k, n - k - 8, n - k - 16, n - k - 24])
    return front[2], back[2]


def test_fuzz_is_not_vacuous(fuzz):
    """Conditions the restatement meets alone: at least 100 supporting records in each of the four orientation classes, at least 20
    events with homology, every tally above zero, and a read and its reverse complement give the same events."""
    seqs, reads, gs = fuzz
    g = gs[21]
    assert 3 <= len(seqs) <= 5 and any("N" in s for _, s in seqs) and 2400 <= len(reads) <= 2600
    res = chimeras_ref.chimera_events(g, reads)
    assert all(v > 0 for v in res.counters.values()), res.counters
    classes = {}
    for r in reads:
        one = chimeras_ref.chimera_events(g, [r])
        if one.counters["supporting"] == 1 and one.counters["records"] == 1:
            o = _orientation(g, r)
            classes[o] = classes.get(o, 0) + 1
    assert len(classes) == 4 and min(classes.values()) >= 100, classes
    assert sum(1 for key in res.events if chimeras_ref.homology(g, *key) > 0) >= 20
    assert {(key[1], key[3]) for key in res.events} == {(L, R), (L, L), (R, R), (R, L)}
    assert sum(1 for lf, hf in res.events.values() if lf and hf) >= 10          # events met from both cells
    for r in reads[:300]:
        a, b = chimeras_ref.chimera_events(g, [r]), chimeras_ref.chimera_events(g, [chimeras_ref.revcomp(r)])
        assert list(a.events) == list(b.events) and [v[::-1] for v in a.events.values()] == list(b.events.values())
        assert a.span == b.span and a.counters == b.counters


@pytest.mark.parametrize("k", [21, 31])
def test_fuzz_twin_equals_restatement(fuzz, k):
    seqs, reads, gs = fuzz
    ix = HostIndex.build_mem(k, [("fuzz", [(name, s.encode()) for name, s in seqs])])
    try:
        res = _both(ix, gs[k], reads)
        assert res.counters["records"] >= len(reads) and res.events
        _both(ix, gs[k], reads[:600], 0)
        _both(ix, gs[k], reads[:600], 8)
    finally:
        ix.close()


def test_writer_text(tmp_path):
    """Hand-written lines: the order is (lo, side_lo, hi, side_hi), positions are 1-based within their sequence, freq is truncated and
    takes the larger span, homology comes from the reference, the header gives the two tallies."""
    k = 21
    seqs = chimera_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    try:
        g = _genome(seqs, k)
        fa, fb, fc, fd, fe, ff = g.first
        (u1, v1, _), (u6, v6, _) = (chimera_cases.along_sites(k)[n] for n in ("one", "six"))
        (_, _, _), (w6, z6, _) = (chimera_cases.turned_sites(k)[n] for n in ("one", "six"))
        x, y = chimera_cases.free_pair(g.text, fe + 450, ff + 150)
        # rows as bk_chimera_record: (lo, hi, sides, lo_first, hi_first, span_lo, span_hi, 0)
        rows = [(ff - 1, ff, 2, 2, 1, 6, 9, 0), (x, y, 3, 1, 0, 0, 2, 0), (x, y, 0, 3, 0, 0, 4, 0), (x, y, 2, 1, 1, 1, 0, 0), (x, y, 1, 0, 5, 10, 10, 0),
                (fe + u6 - 1, ff + v6, 2, 7, 0, 14, 2, 0), (fe + w6 - 1, ff + z6, 0, 1, 1, 0, 0, 0), (fe + u1, ff + v1 - 1, 1, 1, 2, 4, 5, 0), (100, fb + 5, 2, 1, 0, 0, 2, 0)]
        path = str(tmp_path / "x.chimeras.tsv")
        hostlib.write_chimeras_tsv(path, ix, 0, rows, 2, 1, 31, 969)
        text = open(path).read()
        hx, hy = x - fe + 1, y - ff + 1
        want = ["##chimera_max_mismatches=2", "##chimera_min_reads=1", "##chimera_supporting=31", "##chimera_ref_spanning=969",
                "chrom_lo\tpos_lo\tside_lo\tchrom_hi\tpos_hi\tside_hi\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology",
                "craftA\t101\tL\tcraftB\t6\tR\t1\t0\t1\t0\t2\t0.3333\t%d" % chimeras_ref.homology(g, 100, L, fb + 5, R),
                "craftE\t%d\tR\tcraftF\t%d\tL\t1\t2\t3\t4\t5\t0.3750\t1" % (u1 + 1, v1),
                "craftE\t%d\tL\tcraftF\t%d\tR\t7\t0\t7\t14\t2\t0.3333\t6" % (u6, v6 + 1),
                "craftE\t%d\tL\tcraftF\t%d\tL\t3\t0\t3\t0\t4\t0.4285\t0" % (hx, hy),
                "craftE\t%d\tL\tcraftF\t%d\tR\t1\t1\t2\t1\t0\t0.6666\t0" % (hx, hy),
                "craftE\t%d\tR\tcraftF\t%d\tL\t0\t5\t5\t10\t10\t0.3333\t0" % (hx, hy),
                "craftE\t%d\tR\tcraftF\t%d\tR\t1\t0\t1\t0\t2\t0.3333\t0" % (hx, hy),
                "craftE\t%d\tL\tcraftF\t%d\tL\t1\t1\t2\t0\t0\t1.0000\t6" % (w6, z6 + 1),
                "craftE\t1200\tL\tcraftF\t1\tR\t2\t1\t3\t6\t9\t0.2500\t0"]
        assert w6 > u6 and u6 > u1 and x > fe + u6 and x < fe + w6             # (the order of the lines above)
        assert text == "".join(line + "\n" for line in want)
        assert text == chimeras_ref.tsv_text(g, rows, 2, 1, 31, 969)
        hostlib.write_chimeras_tsv(path, ix, 0, [], 0, 7, 0, 12)     # a sample without events: the five lines
        assert open(path).read() == chimeras_ref.tsv_text(g, [], 0, 7, 0, 12) and len(open(path).read().splitlines()) == 5
        assert open(path).read().splitlines()[:4] == ["##chimera_max_mismatches=0", "##chimera_min_reads=7", "##chimera_supporting=0", "##chimera_ref_spanning=12"]
        # both cells in one sequence, a cell outside the file, a cell on a letter that is not ACGT, sides above 3
        for bad in ((fe + 10, fe + 400, 2, 1, 0, 0, 0, 0), (fe + 10, g.cells, 2, 1, 0, 0, 0, 0), (fe + chimera_cases.E_N_RUN[0] + 3, ff + 10, 2, 1, 0, 0, 0, 0),
                    (x, y, 4, 1, 0, 0, 0, 0)):
            with pytest.raises(RuntimeError):
                hostlib.write_chimeras_tsv(path, ix, 0, [bad], 2, 5, 0, 0)
    finally:
        ix.close()
    f = chimeras_ref.freq_text
    assert f(1, 2, 0) == "0.3333" and f(1, 0, 2) == "0.3333" and f(3, 0, 0) == "1.0000" and f(2, 1, 1) == "0.6666"


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--chimera-max-mismatches", "1"], "--chimera-max-mismatches needs --chimeras"),
                        (["--chimera-min-reads", "3"], "--chimera-min-reads needs --chimeras"),
                        (["--chimeras", "--chimera-max-mismatches", "9"], "--chimera-max-mismatches must be between 0 and 8, got 9"),
                        (["--chimeras", "--chimera-max-mismatches", "-1"], "--chimera-max-mismatches must be between 0 and 8, got -1"),
                        (["--chimeras", "--chimera-min-reads", "0"], "--chimera-min-reads must be at least 1, got 0")):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
    r = _run(*base, "--chimeras", "--chimera-min-reads", "x")
    assert r.returncode == 2 and "invalid value 'x' for '--chimera-min-reads'" in r.stderr
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), "--chimeras")
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout
    usage = _run("call", "--help")
    for flag in ("--chimeras", "--chimera-max-mismatches", "--chimera-min-reads", ".chimeras.tsv"):
        assert flag in usage.stdout + usage.stderr, flag


def test_both_libraries_export_the_four_functions():
    names = ("bk_chimeras_enable", "bk_sample_chimeras", "bk_sample_download_chimeras", "bk_sample_download_chimera_span")
    for testing in (False, True):
        lib = _ffi.load(testing=testing)
        assert lib.bk_abi_version() == 8
        for name in names:
            assert hasattr(lib, name) and name in _ffi.SYMBOLS, name
    import ctypes as C
    assert C.sizeof(_ffi.ChimeraConfig) == 8 and C.sizeof(_ffi.ChimeraParams) == 8 and C.sizeof(_ffi.ChimeraSummary) == 72
