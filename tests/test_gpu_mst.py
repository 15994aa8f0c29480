"""--mst on the device: bk_cohort_mst (Boruvka by row blocks: cohort_pairs_kernel, cohort_row_best_kernel and the two component
kernels of bronko_amd/csrc/bk_cohort.hip, merged by the library's host code) against the restatement (tests/mst_ref.py: Kruskal and
a plain Boruvka), exactly, rounds included; block borders through the testing library's BK_COHORT_MST_BLOCK_ROWS; state and errors;
`bronko call --distances --mst` end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, synth
from tests import cohort_ref, helpers, mst_cases, mst_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
INVALID, STATE = -1, -5

SAMPLES = (1, 2, 3, 63, 64, 65, 130)
POSITIONS = (129, 700, 4999)


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


def _tuples(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


def _check(e, kind, n, positions):
    """The cohort is set; the forest of every min_compared against the restatement."""
    for need in mst_cases.needs(positions):
        want_edges, want_near, want_rounds = mst_cases.expected(kind, n, positions, need)
        edges, near, rounds = e.cohort_mst(need)
        assert _tuples(edges) == want_edges, need
        assert _tuples(near) == want_near, need
        assert rounds == want_rounds, need


@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("kind", mst_cases.KINDS)
def test_equals_the_restatement(eng, kind, n, positions):
    eng.cohort_set(mst_cases.case(kind, n, positions)[0])
    _check(eng, kind, n, positions)


@pytest.mark.parametrize("block_rows", [1, 3, 64])
@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("kind", mst_cases.KINDS)
def test_block_borders(eng_testing, monkeypatch, kind, n, positions, block_rows):
    """Row blocks of 1, 3 and 64 rows over slices of 3 words: every round crosses block, tile, slice and chunk borders."""
    monkeypatch.setenv("BK_COHORT_MST_BLOCK_ROWS", str(block_rows))
    monkeypatch.setenv("BK_COHORT_SLICE_WORDS", "3")
    eng_testing.cohort_set(mst_cases.case(kind, n, positions)[0])
    _check(eng_testing, kind, n, positions)


def test_release_library_does_not_read_the_block_variable(eng, monkeypatch):
    assert b"BK_COHORT_MST_BLOCK_ROWS" not in open(_ffi.LIB_PATH, "rb").read()
    assert b"BK_COHORT_MST_BLOCK_ROWS" in open(_ffi.TESTING_LIB_PATH, "rb").read()
    monkeypatch.setenv("BK_COHORT_MST_BLOCK_ROWS", "1")           # (and gives the same forest with it set)
    eng.cohort_set(mst_cases.case("ruler", 65, 700)[0])
    _check(eng, "ruler", 65, 700)


def test_null_outputs_and_the_cohort_stays(eng):
    kind, n, positions = "clonal", 130, 700
    a, want_d, want_c = mst_cases.case(kind, n, positions)
    need = mst_cases.needs(positions)[2]
    want_edges, want_near, want_rounds = mst_cases.expected(kind, n, positions, need)
    eng.cohort_set(a)
    d, c = eng.cohort_distances()
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)
    for nearest, rounds in ((False, False), (True, False), (False, True)):
        edges, near, r = eng.cohort_mst(need, nearest=nearest, rounds=rounds)
        assert _tuples(edges) == want_edges
        assert near is None if not nearest else _tuples(near) == want_near
        assert r is None if not rounds else r == want_rounds
    d, c = eng.cohort_distances()                                # the cohort is as it was, block by block too
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)
    d, c = eng.cohort_distances(60, 10)
    assert np.array_equal(d, want_d[60:70]) and np.array_equal(c, want_c[60:70])
    # exactly n - 1 edges fit
    buf = np.zeros((n - 1, 4), np.uint32)
    n_edges = C.c_uint64(99)
    assert eng._L.bk_cohort_mst(eng.h, 0, buf.ctypes.data_as(C.POINTER(_ffi.MstEdge)), n - 1, C.byref(n_edges), None, None) == 0
    assert _tuples(buf[:n_edges.value]) == mst_cases.expected(kind, n, positions, 0)[0]


def _error(e, rc):
    assert rc != 0
    return rc, e._L.bk_last_error().decode()


def test_errors(eng):
    L, h = eng._L, eng.h
    a, _, _ = mst_cases.case("related", 5, 129)
    buf = np.full((8, 4), 0xdeadbeef, np.uint32)
    eptr = buf.ctypes.data_as(C.POINTER(_ffi.MstEdge))
    n_edges = C.c_uint64(77)
    eng.cohort_clear()
    rc, msg = _error(eng, L.bk_cohort_mst(h, 0, eptr, 8, C.byref(n_edges), None, None))
    assert rc == STATE and "bk_cohort_set" in msg
    rc, msg = _error(eng, L.bk_cohort_mst(None, 0, eptr, 8, C.byref(n_edges), None, None))
    assert rc == INVALID
    eng.cohort_set(a)
    rc, msg = _error(eng, L.bk_cohort_mst(h, 0, None, 8, C.byref(n_edges), None, None))
    assert rc == INVALID and "edges" in msg
    rc, msg = _error(eng, L.bk_cohort_mst(h, 0, eptr, 8, None, None, None))
    assert rc == INVALID and "n_edges" in msg
    near = np.full((5, 3), 0xdeadbeef, np.uint32)
    rounds = C.c_uint32(55)
    for cap in (0, 3):
        rc, msg = _error(eng, L.bk_cohort_mst(h, 0, eptr, cap, C.byref(n_edges), near.ctypes.data_as(C.POINTER(_ffi.MstNearest)), C.byref(rounds)))
        assert rc == INVALID and "cap_edges" in msg, msg
    assert (buf == 0xdeadbeef).all() and (near == 0xdeadbeef).all() and n_edges.value == 77 and rounds.value == 55   # nothing was written
    assert L.bk_cohort_mst(h, 0, eptr, 4, C.byref(n_edges), None, None) == 0
    assert _tuples(buf[:n_edges.value]) == mst_cases.expected("related", 5, 129, 0)[0]
    eng.cohort_clear()
    with pytest.raises(BronkoError) as ei:
        eng.cohort_mst(0)
    assert ei.value.status == STATE


def test_refused_inside_a_sample(eng, oracle, golden_dir):
    a, _, _ = mst_cases.case("related", 65, 4999)
    eng.cohort_set(a)
    want = mst_cases.expected("related", 65, 4999, 0)
    reads = helpers.hpv_reads(2000, 5)
    words, lens = pack_reads(reads, 21)
    buf = np.zeros((64, 4), np.uint32)
    n_edges = C.c_uint64(0)
    eng.sample_begin()
    rc, msg = _error(eng, eng._L.bk_cohort_mst(eng.h, 0, buf.ctypes.data_as(C.POINTER(_ffi.MstEdge)), 64, C.byref(n_edges), None, None))
    assert rc == STATE and "inside a sample" in msg
    eng.push_reads(0, words, lens)
    res = eng.sample_finish(1)
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    try:
        helpers.assert_same_pileup(res, oracle.sample_pileup(ix, [reads]))
    finally:
        ix.close()
    edges, near, rounds = eng.cohort_mst(0)                      # ... and the cohort is as it was
    assert (_tuples(edges), _tuples(near), rounds) == want
    eng.cohort_clear()


def test_a_smaller_cohort_after_a_larger_one_and_on_a_fork(eng):
    shapes = (("ruler", 130, 700), ("clonal", 3, 129), ("related", 64, 129), ("ruler", 130, 700))
    f = eng.fork()
    try:
        for e in (eng, f):
            for kind, n, positions in shapes:
                e.cohort_set(mst_cases.case(kind, n, positions)[0])
                _check(e, kind, n, positions)
        # the fork and its parent own theirs
        eng.cohort_set(mst_cases.case("clonal", 3, 129)[0])
        _check(f, "ruler", 130, 700)
        _check(eng, "clonal", 3, 129)
        f.cohort_clear()
        with pytest.raises(BronkoError) as ei:
            f.cohort_mst(0)
        assert ei.value.status == STATE
        _check(eng, "clonal", 3, 129)
    finally:
        f.close()


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
    """Three HPV16 samples with 0, 3 and 5 planted substitutions (the second with an uncovered stretch) and two SARS-CoV-2 samples."""
    d = tmp_path_factory.mktemp("mst_cli")
    hpv = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    sars = synth.read_fasta_bytes(os.path.join(golden_dir, "4_sarscov2", "wuhan_ref.fasta"))
    paths = {}
    for name, genome, n_sub in (("hpv_a", hpv, 0), ("hpv_b", hpv, 3), ("hpv_c", hpv, 5)):
        gm = _substituted(genome, PLANTED[:n_sub])
        if name == "hpv_b":
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


def _expected_mst(out, stems, positions, breadth):
    letters = np.array([np.frombuffer(_fasta_letters(os.path.join(out, s + ".consensus.fa")), np.uint8) for s in stems])
    assert letters.shape == (len(stems), positions)
    d, c = cohort_ref.distances(letters)
    need = mst_ref.min_compared(breadth, positions)
    edges = mst_ref.kruskal(d, c, need)
    return mst_ref.mst_text(stems, edges, mst_ref.nearest(d, c, need), breadth, need), edges, d


def test_cli_mst_end_to_end(golden_dir, tmp_path, cli_inputs):
    paths, hpv_len, sars_len = cli_inputs
    order = ["hpv_a", "sars_a", "hpv_b", "hpv_c", "sars_b"]
    out = str(tmp_path / "o")
    log = _run_cli(golden_dir, out, [paths[s] for s in order], ["--distances", "--mst"])
    hpv_text, hpv_edges, d = _expected_mst(out, ["hpv_a", "hpv_b", "hpv_c"], hpv_len, 0.9)
    sars_text, sars_edges, _ = _expected_mst(out, ["sars_a", "sars_b"], sars_len, 0.9)
    assert open(os.path.join(out, "HPV16.mst.tsv"), "rb").read() == hpv_text
    assert open(os.path.join(out, "wuhan_ref.mst.tsv"), "rb").read() == sars_text
    assert (int(d[0, 1]), int(d[0, 2]), int(d[1, 2])) == (3, 5, 2)            # the planted distances:
    assert [e[:3] for e in hpv_edges] == [(1, 2, 2), (0, 1, 3)]               # a - b and b - c, not a - c
    lines = hpv_text.decode().splitlines()[3:]
    assert [l.split("\t")[:3] for l in lines] == [["hpv_a", ".", "."], ["hpv_b", "hpv_a", "3"], ["hpv_c", "hpv_b", "2"]]
    assert [e[:3] for e in sars_edges] == [(0, 1, 1)]
    assert "Forest for HPV16: 3 samples, 2 edges, 1 components, the largest of 3 samples, longest edge 3, 1 rounds (" in log
    assert "Forest for wuhan_ref: 2 samples, 1 edges, 1 components, the largest of 2 samples, longest edge 1, 1 rounds (" in log
    assert "Distances for HPV16: 3 samples, largest distance 5, 0 pairs with nothing compared (" in log
    # with --distances alone: the same files but the two forests, and no forest line
    plain = str(tmp_path / "plain")
    log = _run_cli(golden_dir, plain, [paths[s] for s in order], ["--distances"])
    assert "Forest" not in log
    assert set(os.listdir(out)) == set(os.listdir(plain)) | {"HPV16.mst.tsv", "wuhan_ref.mst.tsv"}
    for f in os.listdir(plain):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f


def test_cli_breadth_bound_and_a_skipped_genome(golden_dir, tmp_path, cli_inputs):
    """--mst-min-breadth 0.99: hpv_b's gap keeps it from every edge; a genome with one sample gets no .mst.tsv."""
    paths, hpv_len, _ = cli_inputs
    out = str(tmp_path / "o")
    log = _run_cli(golden_dir, out, [paths[s] for s in ("hpv_a", "hpv_b", "sars_a", "hpv_c")], ["--distances", "--mst", "--mst-min-breadth", "0.99"])
    text, edges, _ = _expected_mst(out, ["hpv_a", "hpv_b", "hpv_c"], hpv_len, 0.99)
    assert open(os.path.join(out, "HPV16.mst.tsv"), "rb").read() == text
    assert text.startswith(b"##mst_min_breadth=0.99\n##mst_min_compared=%d\n" % mst_ref.min_compared(0.99, hpv_len))
    assert all(1 not in e[:2] for e in edges) and b"hpv_b\t.\t.\t.\t" in text
    assert "Skipping distances for wuhan_ref" in log and "Forest for wuhan_ref" not in log
    assert not os.path.exists(os.path.join(out, "wuhan_ref.mst.tsv"))
