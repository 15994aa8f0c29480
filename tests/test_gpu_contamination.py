"""--contamination on the device: cohort_minor_pack_kernel and cohort_explained_kernel (bronko_amd/csrc/bk_cohort.hip) through
bk_cohort_set_minor and bk_cohort_explained against the plain-numpy restatement (tests/contamination_ref.py), exactly; the slice and
chunk borders through the testing library's BK_COHORT_SLICE_WORDS; row blocks, state and errors; `bronko call --contamination` end to
end."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, synth
from tests import cohort_ref, contamination_ref, helpers
from tests.test_gpu_cohort import BRONKO, CASES, GAP, PLANTED, _engine, _error, _fasta_letters, _substituted, _write_fastq

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -5


@functools.lru_cache(maxsize=None)
def _case(n, positions):
    a, m = contamination_ref.cohort(n, positions, 1000 * n + positions)
    ex, sites = contamination_ref.explained(a, m)
    for v in (a, m, ex, sites):
        v.setflags(write=False)
    return a, m, ex, sites


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


def _set(e, a, m):
    e.cohort_set(a)
    e.cohort_set_minor(m)


@pytest.mark.parametrize("n,positions", CASES)
def test_equals_the_restatement(eng, n, positions):
    a, m, want, want_sites = _case(n, positions)
    _set(eng, a, m)
    ex, sites = eng.cohort_explained()
    assert np.array_equal(ex, want) and np.array_equal(sites, want_sites)


@pytest.mark.parametrize("slice_words", [1, 3])
@pytest.mark.parametrize("n,positions", CASES)
def test_slice_and_chunk_borders(eng_testing, monkeypatch, n, positions, slice_words):
    monkeypatch.setenv("BK_COHORT_SLICE_WORDS", str(slice_words))
    a, m, want, want_sites = _case(n, positions)
    _set(eng_testing, a, m)
    ex, sites = eng_testing.cohort_explained()
    assert np.array_equal(ex, want) and np.array_equal(sites, want_sites)


@pytest.mark.parametrize("which", ["release", "testing"])
def test_row_blocks(eng, eng_testing, monkeypatch, which):
    e = eng
    if which == "testing":
        e = eng_testing
        monkeypatch.setenv("BK_COHORT_SLICE_WORDS", "3")
    n, positions = 130, 129
    a, m, want, want_sites = _case(n, positions)
    _set(e, a, m)
    for row0, rows in ((0, 1), (1, 1), (n - 1, 1), (0, n - 1), (1, n - 1), (60, 10), (63, 2), (127, 3)):   # (60, 10), (63, 2), (127, 3): across a tile edge
        ex, sites = e.cohort_explained(row0, rows)
        assert np.array_equal(ex, want[row0:row0 + rows]) and np.array_equal(sites, want_sites[row0:row0 + rows]), (row0, rows)
    blocks = [e.cohort_explained(r, min(50, n - r)) for r in range(0, n, 50)]      # the union of the blocks is the matrix
    assert np.array_equal(np.concatenate([b[0] for b in blocks]), want)
    assert np.array_equal(np.concatenate([b[1] for b in blocks]), want_sites)
    # each output pointer NULL in turn; the other is written, nothing else is
    buf = np.full((10, n), 0xdeadbeef, np.uint32)
    assert e._L.bk_cohort_explained(e.h, 60, 10, buf.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(buf, want[60:70])
    sbuf = np.full(12, 0xdeadbeef, np.uint32)
    assert e._L.bk_cohort_explained(e.h, 60, 10, None, sbuf.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(sbuf[:10], want_sites[60:70]) and (sbuf[10:] == 0xdeadbeef).all()
    assert e._L.bk_cohort_explained(e.h, 0, 1, None, None) == 0


def test_distances_and_mst_are_the_same_before_and_after(eng):
    a, m, want, _ = _case(65, 4999)
    eng.cohort_set(a)
    d0, c0 = eng.cohort_distances()
    edges0, near0, rounds0 = eng.cohort_mst(10)
    eng.cohort_set_minor(m)
    block = eng.cohort_distances(3, 7)                           # the block the distances left is not the explained block's
    ex, _ = eng.cohort_explained()
    assert np.array_equal(ex, want)
    d1, c1 = eng.cohort_distances()
    edges1, near1, rounds1 = eng.cohort_mst(10)
    assert np.array_equal(d0, d1) and np.array_equal(c0, c1) and np.array_equal(block[0], d0[3:10])
    assert np.array_equal(edges0, edges1) and np.array_equal(near0, near1) and rounds0 == rounds1
    want_d, want_c = cohort_ref.distances(a)
    assert np.array_equal(d1, want_d) and np.array_equal(c1, want_c)
    eng.cohort_set_minor(m & 15)                                 # a second call replaces the planes; the upper bits never counted
    assert np.array_equal(eng.cohort_explained()[0], want)


def test_a_new_cohort_drops_the_minor_planes_and_a_fork_owns_its_own(eng):
    big, small = _case(130, 129), _case(5, 129)
    f = eng.fork()
    try:
        for e in (eng, f):
            for a, m, want, want_sites in (big, small, big):
                _set(e, a, m)
                ex, sites = e.cohort_explained()
                assert np.array_equal(ex, want) and np.array_equal(sites, want_sites)
        eng.cohort_set(small[0])                                 # a new cohort: no minor planes, on this engine only
        with pytest.raises(BronkoError) as ei:
            eng.cohort_explained(0, 1)
        assert ei.value.status == STATE and "bk_cohort_set_minor" in str(ei.value)
        assert np.array_equal(f.cohort_explained()[0], big[2])
        eng.cohort_set_minor(small[1])
        assert np.array_equal(eng.cohort_explained()[0], small[2])
        f.cohort_clear()
        with pytest.raises(BronkoError) as ei:
            f.cohort_explained(0, 1)
        assert ei.value.status == STATE
        with pytest.raises(BronkoError) as ei:
            f.cohort_set_minor(big[1])
        assert ei.value.status == STATE
        assert np.array_equal(eng.cohort_explained()[0], small[2])
    finally:
        f.close()


def test_errors_name_their_parameter(eng):
    L, h = eng._L, eng.h
    a, m, want, _ = _case(5, 129)
    mptr = m.ctypes.data_as(C.c_void_p)
    out = np.zeros((5, 5), np.uint32)
    optr = out.ctypes.data_as(C.c_void_p)
    eng.cohort_clear()
    rc, msg = _error(eng, L.bk_cohort_set_minor(h, mptr, 5, 129))
    assert rc == STATE and "bk_cohort_set" in msg
    rc, msg = _error(eng, L.bk_cohort_explained(h, 0, 1, optr, None))
    assert rc == STATE and "bk_cohort_set" in msg
    assert _error(eng, L.bk_cohort_set_minor(None, mptr, 5, 129))[0] == INVALID
    assert _error(eng, L.bk_cohort_explained(None, 0, 1, optr, None))[0] == INVALID
    eng.cohort_set(a)
    rc, msg = _error(eng, L.bk_cohort_explained(h, 0, 1, optr, None))
    assert rc == STATE and "bk_cohort_set_minor" in msg
    for args, word in (((None, 5, 129), "masks"), ((mptr, 4, 129), "n_samples"), ((mptr, 6, 129), "n_samples"), ((mptr, 5, 128), "positions"),
                       ((mptr, 5, 130), "positions")):
        rc, msg = _error(eng, L.bk_cohort_set_minor(h, *args))
        assert rc == INVALID and word in msg, (args[1:], msg)
    eng.cohort_set_minor(m)
    rc, msg = _error(eng, L.bk_cohort_set_minor(h, mptr, 4, 129))   # a refused call leaves the planes as they were
    assert rc == INVALID
    for row0, rows, word in ((0, 0, "n_rows"), (5, 1, "row0"), (4, 2, "n_rows"), (0, 6, "n_rows"), (1 << 63, 1 << 63, "row0")):
        rc, msg = _error(eng, L.bk_cohort_explained(h, row0, rows, optr, None))
        assert rc == INVALID and word in msg, (row0, rows, msg)
    assert not out.any()                                         # (nothing was written by the refused calls)
    assert np.array_equal(eng.cohort_explained()[0], want)
    eng.cohort_clear()


def test_a_sample_after_the_cohort_matches_its_pileup(eng, oracle, golden_dir):
    a, m, want, want_sites = _case(65, 4999)
    _set(eng, a, m)
    eng.cohort_explained()
    reads = helpers.hpv_reads(2000, 5)
    words, lens = pack_reads(reads, 21)
    eng.sample_begin()
    rc, msg = _error(eng, eng._L.bk_cohort_set_minor(eng.h, m.ctypes.data_as(C.c_void_p), 65, 4999))
    assert rc == STATE and "inside a sample" in msg
    rc, msg = _error(eng, eng._L.bk_cohort_explained(eng.h, 0, 1, None, None))
    assert rc == STATE and "inside a sample" in msg
    eng.push_reads(0, words, lens)
    res = eng.sample_finish(1)
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    try:
        helpers.assert_same_pileup(res, oracle.sample_pileup(ix, [reads]))
    finally:
        ix.close()
    ex, sites = eng.cohort_explained()                           # ... and the cohort is as it was
    assert np.array_equal(ex, want) and np.array_equal(sites, want_sites)
    eng.cohort_clear()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
STEMS = ["mix_pure", "mix_planted", "mix_mixture", "mix_gap"]


@pytest.fixture(scope="module")
def cli_inputs(golden_dir, tmp_path_factory):
    """Four samples of HPV16: a pure one, one with 5 planted substitutions, 80 % reads of the first and 20 % of the second, one with
    an uncovered stretch."""
    d = tmp_path_factory.mktemp("contamination_cli")
    hpv = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    planted = _substituted(hpv, PLANTED)
    reads = {
        "mix_pure": synth.codes_to_ascii(synth.single_end_codes(hpv, 4000, 150, 700)),
        "mix_planted": synth.codes_to_ascii(synth.single_end_codes(planted, 4000, 150, 701)),
        "mix_mixture": synth.codes_to_ascii(synth.single_end_codes(hpv, 4800, 150, 702)) + synth.codes_to_ascii(synth.single_end_codes(planted, 1200, 150, 703)),
        "mix_gap": [],
    }
    for part, (lo, hi) in enumerate(((0, GAP[0]), (GAP[1], len(hpv)))):
        reads["mix_gap"] += synth.codes_to_ascii(synth.single_end_codes(hpv[lo:hi], 4000 * (hi - lo) // len(hpv), 150, 704 + part))
    paths = {}
    for name in STEMS:
        paths[name] = str(d / (name + ".fastq"))
        _write_fastq(paths[name], reads[name])
    return paths, len(hpv)


def _run(golden_dir, out, reads, extra):
    res = subprocess.run([BRONKO, "call", "-d", os.path.join(golden_dir, "hpv.bkdb"), "-r"] + reads + ["-o", out, "-t", "8", "--pileup", "--consensus"] + extra,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def _pileup_counts(path):
    """(fwd, rev): the four counts a position of either strand of a sample's pileup file (columns A C G T and a c g t)."""
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["reference", "index", "ref", "A", "C", "G", "T", "a", "c", "g", "t"]
    rows = np.array([[int(v) for v in ln.split("\t")[3:]] for ln in lines[1:]], np.uint64)
    return rows[:, :4].reshape(-1), rows[:, 4:].reshape(-1)


def test_cli_contamination_end_to_end(golden_dir, tmp_path, cli_inputs):
    paths, hpv_len = cli_inputs
    out, plain = str(tmp_path / "o"), str(tmp_path / "plain")
    log = _run(golden_dir, out, [paths[s] for s in STEMS], ["--distances", "--contamination"])
    plain_log = _run(golden_dir, plain, [paths[s] for s in STEMS], ["--distances"])
    letters = np.array([np.frombuffer(_fasta_letters(os.path.join(out, s + ".consensus.fa")), np.uint8) for s in STEMS])
    assert letters.shape == (4, hpv_len)
    masks = np.array([contamination_ref.present_masks(*_pileup_counts(os.path.join(out, s + ".tsv")), 10, 0.03)[0] for s in STEMS])
    d, c = cohort_ref.distances(letters)
    ex, sites = contamination_ref.explained(letters, masks)
    want = {"HPV16.explained.tsv": contamination_ref.explained_text(STEMS, ex),
            "HPV16.contamination.tsv": contamination_ref.contamination_text(STEMS, d, c, ex, sites, 10, 0.03, 3, 0.75),
            "HPV16.mixture.tsv": contamination_ref.mixture_text(STEMS, d, ex, sites, 10, 0.03, 3, 0.75)}
    for name, text in want.items():
        assert open(os.path.join(out, name), "rb").read() == text, name
    # the mixture carries the planted sample's five alleles and is the only flagged recipient; the pure samples explain nothing
    assert int(ex[2, 1]) == int(d[2, 1]) == 5
    flagged, _, counts = contamination_ref.scan(d, ex, 3, 0.75)
    assert flagged == [(2, 1)] and counts == [0, 0, 1, 0]
    assert not ex[0].any() and not ex[1].any() and not ex[3].any()
    assert "Minor alleles: " in log and " mixed positions, " in log and "Minor alleles" not in plain_log
    assert "Contamination for HPV16: 4 samples, 1 flagged pairs, 1 samples flagged at least once, largest explained 5" in log
    assert "Contamination" not in plain_log
    # every other file is what it is without the flag, and the file set without the flag is unchanged
    assert set(os.listdir(out)) == set(os.listdir(plain)) | set(want)
    assert set(os.listdir(plain)) == {s + ext for s in STEMS for ext in (".vcf", ".tsv", ".consensus.fa")} | {"bronko_overview.tsv", "HPV16.distances.tsv", "HPV16.compared.tsv"}
    for f in os.listdir(plain):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f


def test_cli_one_sample_genome_is_skipped(golden_dir, tmp_path, cli_inputs):
    paths, _ = cli_inputs
    out = str(tmp_path / "o")
    log = _run(golden_dir, out, [paths["mix_mixture"]], ["--distances", "--contamination"])
    assert "Skipping distances for HPV16 (1 sample selected it, at least 2 are compared)" in log and "Contamination for" not in log
    assert "Minor alleles: " in log
    assert not [f for f in os.listdir(out) if f.startswith("HPV16.")]
