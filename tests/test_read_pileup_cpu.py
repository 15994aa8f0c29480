"""`bronko call --read-pileup` without a GPU: the host twin (bronko_amd/host/read_pileup.cpp through bh_read_pileup_count and
bh_write_read_pileup_tsv) against the Python restatement of the rule (tests/read_pileup_ref.py) -- every counter of every cell on
rider_fuzz's random cases and on the crafted two-sequence genome, the TSV text byte for byte --, what single crafted records are meant
to show, and the argument errors of `bronko call`.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import haplotype_cases, indel_cases, indels_ref, linkage_ref, read_pileup_ref, rider_fuzz
from tests.linkage_cases import N_LEN, START

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
ENDS = (0, 1, 10, 74, 75, 76, 255)                                 # none; N_LEN = 150 is 2 E for 75: every cell from there on


def _both(ix, g, reads, M, E):
    """The twin's and the restatement's cells of the same reads; asserts that they are equal."""
    raw, _ = hostlib.link_rows(ix, 0, reads, M)
    rows, _ = linkage_ref.link_rows(g, reads, M)
    want = read_pileup_ref.read_pileup(g, rows, E)
    got = hostlib.read_pileup_count(ix, 0, raw, E)
    assert got.shape == want.shape and np.array_equal(got, want), (M, E, np.argwhere(got != want)[:5].tolist())
    covered, bases = read_pileup_ref.summary(want, rows)          # the sum of fwd + rev is the sum of the rows' lengths
    assert bases == sum(r[1] for r in rows)
    return rows, want


@pytest.fixture(scope="module", params=[21, 31])
def crafted(request):
    k = request.param
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    yield k, ix, g, seqs, haplotype_cases.crafted_cases(k)
    ix.close()


def test_crafted_records_twin_equals_restatement(crafted):
    k, ix, g, seqs, cases = crafted
    reads = [r for _, r in cases]
    for M in (0, 2, 8):
        for E in ENDS:
            rows, want = _both(ix, g, reads, M, E)
            assert (want[:, 8:].sum() == 0) == (E == 0)
            if E >= 128:                                           # above every row's length: near is fwd + rev
                assert np.array_equal(want[:, 8:], want[:, :4] + want[:, 4:8])
    assert {r[2] for r in rows} == {0, 1} and g.seq_of(max(r[0] for r in rows)) == 1   # both strands, both sequences
    for label, read in cases:                                      # ... and one by one, so that a difference names its record
        _both(ix, g, [read], 8, 10)
    _both(ix, g, [], 8, 10)
    with pytest.raises(RuntimeError) as ei:
        hostlib.read_pileup_count(ix, 0, hostlib.link_rows(ix, 0, reads, 8)[0], 256)
    assert "256" in str(ei.value)


def test_single_records_are_what_they_are_meant_to_be(crafted):
    k, ix, g, seqs, cases = crafted
    by = dict(cases)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    for label, strand in (("mm_8", 0), ("mm_8/rc", 1)):
        for E in (0, 41, 42, 255):
            rows, got = _both(ix, g, [by[label]], 8, E)
            assert len(rows) == 1 and rows[0][:3] == (START, N_LEN, strand) and len(rows[0][3]) == 8
            assert (got[:START] == 0).all() and (got[START + N_LEN:] == 0).all()
            for c in range(START, START + N_LEN):
                off = c - START
                b = (code[g.text[c]] + 1) % 4 if off in range(40, 104, 9) else code[g.text[c]]
                want = [0] * 12
                want[4 * strand + b] = 1
                want[8 + b] = 1 if min(off, N_LEN - 1 - off) < E else 0
                assert got[c].tolist() == want, (label, E, c)
            # the substitution at offset 40 is near an end from E = 41 on, the one at offset 103 (46 from the last cell) from E = 47 on
            assert got[START + 40, 8:].sum() == (1 if E >= 41 else 0) and got[START + 103, 8:].sum() == (1 if E >= 47 else 0)


def test_rows_at_the_borders_of_the_sequences(crafted):
    """A row from a sequence's first cell, one to its last, on the last sequence too: the -1 of that one lands behind the last cell."""
    k, ix, g, seqs, _ = crafted
    a, b = seqs[0][1], seqs[1][1]
    reads = [a[:N_LEN], indels_ref.revcomp(a[len(a) - N_LEN:]), b[:N_LEN], b[len(b) - N_LEN:], indels_ref.revcomp(b[len(b) - 2 * k:])]
    rows, want = _both(ix, g, reads, 8, 10)
    assert {(r[0], r[0] + r[1]) for r in rows} >= {(len(a) - N_LEN, len(a)), (len(a) + len(b) - N_LEN, g.cells), (g.cells - 2 * k, g.cells)}
    assert want[g.cells - 1, :8].sum() == 2 and want[g.cells - 1, 8:].sum() == 2 and want[len(a) - 1, 4:8].sum() == 1
    for E in (k - 1, k, k + 1):                                    # the row of 2 k bases: 2 E - 2, 2 E and 2 E + 2
        _both(ix, g, reads, 8, E)


def test_rows_of_length_two_e_and_one_less_and_one_more(crafted):
    k, ix, g, seqs, _ = crafted
    a = seqs[0][1]
    E = k + 3
    # substitutions between the two anchor k-mers: on the last cell that is near the first end, the first that is not, the last that is not
    reads = [indel_cases.mut_read(a, START + 7 * i, n, subs=tuple(sorted({E - 1, E, n - E - 1})) if n > 2 * E else (k + 1, k + 3))
             for i, n in enumerate((2 * E - 1, 2 * E, 2 * E + 1, 2 * E + 2))]
    reads += [indels_ref.revcomp(r) for r in reads]
    rows, want = _both(ix, g, reads, 8, E)
    assert sorted(r[1] for r in rows) == sorted([2 * E - 1, 2 * E, 2 * E + 1, 2 * E + 2] * 2)
    for E2 in (0, E - 1, E + 1, 255):
        _both(ix, g, reads, 8, E2)
    one = read_pileup_ref.read_pileup(g, [(START, 2 * E + 1, 0, ())], E)
    assert one[START:START + 2 * E + 1, 8:].sum(axis=1).tolist() == [1] * E + [0] + [1] * E


def test_fuzz_cases_twin_equals_restatement():
    ran, rows_seen, several = 0, 0, 0
    for it in range(40):
        case = rider_fuzz.make_case(rider_fuzz.SEED, it)
        if case is None:
            continue
        g = case.genome()
        ix = HostIndex.build_mem(case.k, case.files())
        try:
            for E in (ENDS[it % len(ENDS)], 10):
                rows, _ = _both(ix, g, case.reads_seen(), case.link_M, E)
        finally:
            ix.close()
        ran, rows_seen, several = ran + 1, rows_seen + len(rows), several + (len(case.seqs) > 1)
    assert ran >= 30 and rows_seen > 1000 and several >= 5, (ran, rows_seen, several)


def test_tsv_text(crafted, tmp_path):
    k, ix, g, seqs, cases = crafted
    names, letters = [name for name, _ in seqs], [s for _, s in seqs]
    assert " " in names[1] and "N" in letters[0]
    for M, E in ((8, 10), (2, 0), (0, 255)):
        rows, counts = _both(ix, g, [r for _, r in cases], M, E)
        want = read_pileup_ref.tsv_text(names, letters, counts, M, E)
        path = str(tmp_path / ("p_%d_%d.tsv" % (M, E)))
        got = hostlib.write_read_pileup_tsv(path, ix, 0, counts, M, E)
        assert open(path).read() == want and got == read_pileup_ref.summary(counts, rows), (M, E)
    lines = want.splitlines()
    assert lines[:2] == ["##read_pileup_max_mismatches=0", "##read_pileup_end=255"] and lines[2].split("\t") == read_pileup_ref.HEADER
    assert len(lines) == 3 + g.cells                               # one line per position, zero-cover positions included
    assert lines[3].split("\t")[:3] == [names[0], "1", letters[0][0]] and lines[3 + len(letters[0])].split("\t")[:2] == [names[1], "1"]
    assert lines[3 + 1305].split("\t")[2:] == ["N"] + ["0"] * 12   # a position of the stretch of N
    assert read_pileup_ref.HEADER[:11] == "reference index ref A C G T a c g t".split()   # --pileup's columns
    empty = np.zeros((g.cells, 12), np.uint32)
    path = str(tmp_path / "empty.tsv")
    assert hostlib.write_read_pileup_tsv(path, ix, 0, empty) == (0, 0) and open(path).read() == read_pileup_ref.tsv_text(names, letters, empty)
    with pytest.raises(RuntimeError):
        hostlib.write_read_pileup_tsv(path, ix, 0, empty[:-1])


def _run(*args):
    return subprocess.run([BRONKO] + list(args), capture_output=True, text=True)


def test_call_argument_errors(golden_dir, sars_paths, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    ok = str(tmp_path / "ok.bed")
    open(ok, "w").write("HPV16REF\t2000\t2300\tampA\n")
    db = os.path.join(golden_dir, "hpv.bkdb")
    base = ["call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")]
    P = ["--read-pileup"]
    for extra, words in ((["--read-pileup-end", "5"], ["--read-pileup-end", "needs --read-pileup"]),
                         (["--read-pileup-max-mismatches", "3"], ["--read-pileup-max-mismatches", "needs --read-pileup"]),
                         (P + ["--read-pileup-end", "256"], ["--read-pileup-end", "256"]), (P + ["--read-pileup-end", "-1"], ["--read-pileup-end"]),
                         (P + ["--read-pileup-max-mismatches", "9"], ["--read-pileup-max-mismatches", "9"]),
                         (P + ["--read-pileup-max-mismatches", "-1"], ["--read-pileup-max-mismatches"]),
                         (P + ["--linkage", "--link-max-mismatches", "3"], ["--link-max-mismatches (3)", "--read-pileup-max-mismatches (8)"]),
                         (P + ["--linkage", "--read-pileup-max-mismatches", "2"], ["--link-max-mismatches (8)", "--read-pileup-max-mismatches (2)"]),
                         (P + ["--codons", ok, "--codon-max-mismatches", "3"], ["--codon-max-mismatches (3)", "--read-pileup-max-mismatches (8)"]),
                         (P + ["--hap-window", "100", "--read-pileup-max-mismatches", "2"], ["--hap-max-mismatches (8)", "--read-pileup-max-mismatches (2)"])):
        r = _run(*base, *extra)
        assert r.returncode == 1 and "ERROR" in r.stdout and all(w in r.stdout for w in words) and "no HIP device" not in r.stdout, (extra, r.stdout)
    assert _run(*base, *P, "--read-pileup-end", "x").returncode == 2
    assert _run(*base, *P, "--read-pileup-max-mismatches", "").returncode == 2
    two = str(tmp_path / "two")
    assert _run("build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", two).returncode == 0
    r = _run("call", "-d", two + ".bkdb", "-r", fq, "-o", str(tmp_path / "o2"), *P)
    assert r.returncode == 1 and "ERROR" in r.stdout and "one genome file" in r.stdout and "no HIP device" not in r.stdout, r.stdout


def test_help_names_the_options():
    r = _run("call", "--help")
    text = r.stdout + r.stderr
    assert all(w in text for w in ("--read-pileup ", "--read-pileup-end E", "--read-pileup-max-mismatches M", ".read_pileup.tsv")), text[-2000:]


def test_both_libraries_are_abi_version_8_and_export_the_two_functions():
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        assert L.bk_abi_version() == 8 and hasattr(L, "bk_sample_read_pileup") and hasattr(L, "bk_sample_download_read_pileup")
    assert {"bk_sample_read_pileup", "bk_sample_download_read_pileup"} <= set(_ffi.SYMBOLS)
    import ctypes as C
    assert C.sizeof(_ffi.ReadPileupCell) == 48 and C.sizeof(_ffi.ReadPileupSummary) == 40
