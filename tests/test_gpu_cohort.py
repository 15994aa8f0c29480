"""--distances on the device: cohort_pack_kernel and cohort_pairs_kernel (bronko_amd/csrc/bk_cohort.hip) through bk_cohort_set,
bk_cohort_distances and bk_cohort_clear against the plain-numpy restatement (tests/cohort_ref.py), exactly; the slice and chunk
borders through the testing library's BK_COHORT_SLICE_WORDS; row blocks, state and errors; `bronko call --distances` end to end."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, synth
from tests import cohort_ref, helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
INVALID, STATE = -1, -5

# the tail word, the word border, unaligned row starts (odd lengths); tile edges and a partial tile in both directions
POSITIONS = (1, 63, 64, 65, 127, 128, 129, 4999)
SAMPLES = (1, 2, 3, 63, 64, 65, 130)
CASES = sorted(set([(n, 129) for n in SAMPLES] + [(5, p) for p in POSITIONS] + [(65, 4999), (130, 65), (64, 64)]))


@functools.lru_cache(maxsize=None)
def _case(n, positions):
    a = cohort_ref.cohort(n, positions, 1000 * n + positions)
    a.setflags(write=False)
    d, c = cohort_ref.distances(a)
    d.setflags(write=False)
    c.setflags(write=False)
    return a, d, c


def _engine(oracle, golden_dir, testing):
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    _ffi.use_testing_library(testing)
    try:
        return ix, helpers.engine_from_oracle_index(ix)
    finally:
        _ffi.use_testing_library(False)


@pytest.fixture(scope="module")
def eng(oracle, golden_dir):
    ix, e = _engine(oracle, golden_dir, False)
    yield e
    e.close()
    ix.close()


@pytest.fixture(scope="module")
def eng_testing(oracle, golden_dir):
    ix, e = _engine(oracle, golden_dir, True)
    yield e
    e.close()
    ix.close()


def _error(e, rc):
    assert rc != 0
    return rc, e._L.bk_last_error().decode()


@pytest.mark.parametrize("n,positions", CASES)
def test_equals_the_restatement(eng, n, positions):
    a, want_d, want_c = _case(n, positions)
    eng.cohort_set(a)
    d, c = eng.cohort_distances()
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


@pytest.mark.parametrize("slice_words", [1, 3])
@pytest.mark.parametrize("n,positions", CASES)
def test_slice_and_chunk_borders(eng_testing, monkeypatch, n, positions, slice_words):
    """Slices and LDS chunks of 1 and of 3 words: every border is crossed, every pair's sums are accumulated over all slices."""
    monkeypatch.setenv("BK_COHORT_SLICE_WORDS", str(slice_words))
    a, want_d, want_c = _case(n, positions)
    eng_testing.cohort_set(a)
    d, c = eng_testing.cohort_distances()
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


def test_release_library_does_not_read_the_slice_variable(eng, monkeypatch):
    assert b"BK_COHORT_SLICE_WORDS" not in open(_ffi.LIB_PATH, "rb").read()
    assert b"BK_COHORT_SLICE_WORDS" in open(_ffi.TESTING_LIB_PATH, "rb").read()
    monkeypatch.setenv("BK_COHORT_SLICE_WORDS", "1")             # (and gives the same numbers with it set)
    a, want_d, want_c = _case(65, 4999)
    eng.cohort_set(a)
    d, c = eng.cohort_distances()
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


@pytest.mark.parametrize("which", ["release", "testing"])
def test_row_blocks(eng, eng_testing, monkeypatch, which):
    e = eng
    if which == "testing":
        e = eng_testing
        monkeypatch.setenv("BK_COHORT_SLICE_WORDS", "3")
    n, positions = 130, 129
    a, want_d, want_c = _case(n, positions)
    e.cohort_set(a)
    for row0, rows in ((0, 1), (1, 1), (n - 1, 1), (0, n - 1), (1, n - 1), (60, 10), (63, 2), (127, 3)):   # (60, 10), (63, 2), (127, 3): across a tile edge
        d, c = e.cohort_distances(row0, rows)
        assert np.array_equal(d, want_d[row0:row0 + rows]) and np.array_equal(c, want_c[row0:row0 + rows]), (row0, rows)
    blocks = [e.cohort_distances(r, min(50, n - r)) for r in range(0, n, 50)]      # the union of the blocks is the matrix
    assert np.array_equal(np.concatenate([b[0] for b in blocks]), want_d)
    assert np.array_equal(np.concatenate([b[1] for b in blocks]), want_c)
    # each output pointer NULL in turn; the other is written, nothing else is
    for null_diff in (True, False):
        buf = np.full((10, n), 0xdeadbeef, np.uint32)
        ptr = buf.ctypes.data_as(C.c_void_p)
        rc = e._L.bk_cohort_distances(e.h, 60, 10, None if null_diff else ptr, ptr if null_diff else None)
        assert rc == 0
        assert np.array_equal(buf, (want_c if null_diff else want_d)[60:70])
    assert e._L.bk_cohort_distances(e.h, 0, 1, None, None) == 0


def test_a_smaller_cohort_after_a_larger_one_and_on_a_fork(eng):
    big = _case(130, 129)
    small = _case(3, 129)
    narrow = _case(5, 63)
    f = eng.fork()
    try:
        for e in (eng, f):
            for a, want_d, want_c in (big, small, narrow, big):
                e.cohort_set(a)
                d, c = e.cohort_distances()
                assert np.array_equal(d, want_d) and np.array_equal(c, want_c)
        # the fork and its parent own theirs: another cohort on one leaves the other's as it is
        eng.cohort_set(small[0])
        d, c = f.cohort_distances()
        assert np.array_equal(d, big[1]) and np.array_equal(c, big[2])
        f.cohort_clear()
        d, c = eng.cohort_distances()
        assert np.array_equal(d, small[1]) and np.array_equal(c, small[2])
        with pytest.raises(BronkoError) as ei:
            f.cohort_distances(0, 1)
        assert ei.value.status == STATE
        f2 = eng.fork()                                          # a fork has none of its parent's
        try:
            with pytest.raises(BronkoError) as ei:
                f2.cohort_distances(0, 1)
            assert ei.value.status == STATE
        finally:
            f2.close()
    finally:
        f.close()


def test_clear_and_errors(eng):
    L, h = eng._L, eng.h
    a, want_d, _ = _case(5, 129)
    one = np.zeros(8, np.uint8).ctypes.data_as(C.c_void_p)
    out = np.zeros((5, 5), np.uint32)
    optr = out.ctypes.data_as(C.c_void_p)
    eng.cohort_clear()
    eng.cohort_clear()                                           # fine without a cohort
    rc, msg = _error(eng, L.bk_cohort_distances(h, 0, 1, optr, None))
    assert rc == STATE and "bk_cohort_set" in msg
    for args, word in (((None, 1, 1), "letters"), ((one, 0, 1), "n_samples"), ((one, (1 << 20) + 1, 1), "n_samples"),
                       ((one, 1, 0), "positions"), ((one, 1, 1 << 32), "positions")):
        rc, msg = _error(eng, L.bk_cohort_set(h, *args))
        assert rc == INVALID and word in msg, (args[1:], msg)
    rc, msg = _error(eng, L.bk_cohort_set(None, one, 1, 1))
    assert rc == INVALID
    eng.cohort_set(a)
    rc, msg = _error(eng, L.bk_cohort_set(h, one, 0, 1))         # a call refused for its arguments leaves the cohort as it was
    assert rc == INVALID
    for row0, rows, word in ((0, 0, "n_rows"), (5, 1, "row0"), (4, 2, "n_rows"), (0, 6, "n_rows"), (1 << 63, 1 << 63, "row0")):
        rc, msg = _error(eng, L.bk_cohort_distances(h, row0, rows, optr, None))
        assert rc == INVALID and word in msg, (row0, rows, msg)
    assert not out.any()                                         # (nothing was written by the refused calls)
    d, _ = eng.cohort_distances()
    assert np.array_equal(d, want_d)
    eng.cohort_clear()
    with pytest.raises(BronkoError) as ei:
        eng.cohort_distances(0, 1)
    assert ei.value.status == STATE


def test_a_sample_after_a_cohort_matches_its_pileup(eng, oracle, golden_dir):
    """The cohort touches no sample state, a sample none of the cohort's; inside a sample the cohort calls are refused."""
    a, want_d, want_c = _case(65, 4999)
    eng.cohort_set(a)
    eng.cohort_distances()
    reads = helpers.hpv_reads(2000, 5)
    words, lens = pack_reads(reads, 21)
    eng.sample_begin()
    rc, msg = _error(eng, eng._L.bk_cohort_set(eng.h, a.ctypes.data_as(C.c_void_p), 65, 4999))
    assert rc == STATE and "inside a sample" in msg
    rc, msg = _error(eng, eng._L.bk_cohort_distances(eng.h, 0, 1, None, None))
    assert rc == STATE and "inside a sample" in msg
    eng.push_reads(0, words, lens)
    res = eng.sample_finish(1)
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    try:
        helpers.assert_same_pileup(res, oracle.sample_pileup(ix, [reads]))
    finally:
        ix.close()
    d, c = eng.cohort_distances()                                # ... and the cohort is as it was
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)
    eng.cohort_clear()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
GAP = (3000, 3600)                                               # no read of the second HPV sample covers these positions
PLANTED = (1000, 2500, 5000, 6000, 7000)                         # well covered, far from the gap and from each other


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def _substituted(g, positions):
    g = bytearray(g)
    for p in positions:
        g[p] = b"ACGT"[(b"ACGT".index(g[p]) + 1) % 4]
    return bytes(g)


def _fasta_letters(path):
    return b"".join(line.strip() for line in open(path, "rb") if not line.startswith(b">"))


@pytest.fixture(scope="module")
def cli_inputs(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("cohort_cli")
    hpv = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    sars = synth.read_fasta_bytes(os.path.join(golden_dir, "4_sarscov2", "wuhan_ref.fasta"))
    paths = {}
    for name, genome, n_sub in (("hpv_a", hpv, 0), ("hpv_b", hpv, 3), ("hpv_c", hpv, 5)):
        gm = _substituted(genome, PLANTED[:n_sub])
        if name == "hpv_b":                                      # reads of either side of the gap: none reaches into it
            reads = []
            for part, (lo, hi) in enumerate(((0, GAP[0]), (GAP[1], len(gm)))):
                reads += synth.codes_to_ascii(synth.single_end_codes(gm[lo:hi], 4000 * (hi - lo) // len(gm), 150, 820 + part))
        else:
            reads = synth.codes_to_ascii(synth.single_end_codes(gm, 4000, 150, 800 + n_sub))
        paths[name] = str(d / (name + ".fastq"))
        _write_fastq(paths[name], reads)
    for name, seed in (("sars_a", 900), ("sars_b", 901)):
        gm = _substituted(sars, (2000 + 100 * seed % 5000,) if name == "sars_b" else ())
        paths[name] = str(d / (name + ".fastq"))
        _write_fastq(paths[name], synth.codes_to_ascii(synth.single_end_codes(gm, 6000, 150, seed)))
    return paths, len(hpv), len(sars)


def _run_cli(golden_dir, out, reads, extra):
    genomes = [os.path.join(golden_dir, "HPV16.fa"), os.path.join(golden_dir, "4_sarscov2", "wuhan_ref.fasta")]
    res = subprocess.run([BRONKO, "call", "-g"] + genomes + ["-r"] + reads + ["-o", out, "-t", "8", "--consensus"] + extra, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def _expected_files(out, genome, stems, positions, threshold=None, min_breadth=0.9):
    letters = np.array([np.frombuffer(_fasta_letters(os.path.join(out, s + ".consensus.fa")), np.uint8) for s in stems])
    assert letters.shape == (len(stems), positions)
    d, c = cohort_ref.distances(letters)
    files = {genome + ".distances.tsv": cohort_ref.matrix_text(stems, d), genome + ".compared.tsv": cohort_ref.matrix_text(stems, c)}
    if threshold is not None:
        number, size = cohort_ref.clusters(d, c, positions, threshold, min_breadth)
        files[genome + ".clusters.tsv"] = cohort_ref.clusters_text(stems, number, size, threshold, min_breadth)
    return files, d, c


def test_cli_distances_end_to_end(golden_dir, tmp_path, cli_inputs):
    paths, hpv_len, sars_len = cli_inputs
    order = ["hpv_a", "sars_a", "hpv_b", "hpv_c", "sars_b"]      # (the groups keep the command line's order)
    out = str(tmp_path / "o")
    log = _run_cli(golden_dir, out, [paths[s] for s in order], ["--distances", "--clusters", "3"])
    hpv_files, d, c = _expected_files(out, "HPV16", ["hpv_a", "hpv_b", "hpv_c"], hpv_len, 3)
    sars_files, _, _ = _expected_files(out, "wuhan_ref", ["sars_a", "sars_b"], sars_len, 3)
    for name, want in list(hpv_files.items()) + list(sars_files.items()):
        assert open(os.path.join(out, name), "rb").read() == want, name
    assert (int(d[0, 1]), int(d[0, 2]), int(d[1, 2])) == (3, 5, 2)            # the planted distances
    assert c[0, 1] <= hpv_len - (GAP[1] - GAP[0]) < c[0, 2]                   # the gap is not compared
    assert hpv_files["HPV16.clusters.tsv"].endswith(b"hpv_a\t1\t3\nhpv_b\t1\t3\nhpv_c\t1\t3\n")   # a-c are 5 apart, joined through b
    assert "Distances for HPV16: 3 samples, largest distance 5, 0 pairs with nothing compared, 1 clusters, the largest of 3 samples" in log
    assert "Distances for wuhan_ref: 2 samples" in log and "Skipping distances" not in log
    # without the flags: the same files but those of the cohort
    plain = str(tmp_path / "plain")
    log = _run_cli(golden_dir, plain, [paths[s] for s in order], [])
    assert "Distances" not in log
    assert set(os.listdir(out)) == set(os.listdir(plain)) | set(hpv_files) | set(sars_files)
    for f in os.listdir(plain):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f


def test_cli_one_sample_group_is_skipped(golden_dir, tmp_path, cli_inputs):
    paths, _, sars_len = cli_inputs
    out = str(tmp_path / "o")
    log = _run_cli(golden_dir, out, [paths[s] for s in ("sars_a", "hpv_a", "sars_b")], ["--distances"])
    assert "Skipping distances for HPV16 (1 sample selected it, at least 2 are compared)" in log
    sars_files, d, _ = _expected_files(out, "wuhan_ref", ["sars_a", "sars_b"], sars_len)
    for name, want in sars_files.items():
        assert open(os.path.join(out, name), "rb").read() == want, name
    assert d[0, 1] == 1
    assert not [f for f in os.listdir(out) if f.startswith("HPV16.") or f.endswith(".clusters.tsv")]
