"""--distances without a GPU: the host twin of the cohort kernels, the clusterer and the three writers (bronko_amd/host/cohort.cpp)
against the plain-numpy restatement (tests/cohort_ref.py), and the argument checks of the three flags."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import hostlib
from tests import cohort_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")

# the tail word, the word border, unaligned row starts (odd lengths); tile edges and a partial tile in both directions
POSITIONS = (1, 63, 64, 65, 127, 128, 129, 4999)
SAMPLES = (1, 2, 3, 63, 64, 65, 130)


def _cases():
    out = [(n, 129) for n in SAMPLES] + [(5, p) for p in POSITIONS] + [(65, 4999)]
    return sorted(set(out))


@pytest.mark.parametrize("n,positions", _cases())
def test_host_twin_equals_the_restatement(n, positions):
    a = cohort_ref.cohort(n, positions, 1000 * n + positions)
    want_d, want_c = cohort_ref.distances(a)
    for threads in (1, 16):
        d, c = hostlib.cohort_distances(a, threads=threads)
        assert np.array_equal(d, want_d) and np.array_equal(c, want_c)
    assert np.array_equal(want_d, want_d.T) and np.array_equal(want_c, want_c.T) and not want_d.diagonal().any()
    base = np.isin(a, np.frombuffer(b"ACGT", np.uint8))
    assert np.array_equal(want_c.diagonal(), base.sum(axis=1))
    if n >= 3:                                                   # the all-N sample shares no base with anyone: 0 / 0
        assert not want_c[1].any() and not want_d[1].any()
    if n >= 2:                                                   # the two identical samples
        assert want_d[0, n - 1] == 0 and want_c[0, n - 1] == want_c[0, 0]
    if n >= 5:                                                   # the two that differ everywhere
        assert want_d[2, 3] == want_c[2, 3] == positions


def test_host_twin_row_blocks():
    a = cohort_ref.cohort(65, 129, 7)
    want_d, want_c = cohort_ref.distances(a)
    for row0, rows in ((0, 1), (1, 1), (64, 1), (60, 5), (0, 65)):
        d, c = hostlib.cohort_distances(a, row0, rows)
        assert np.array_equal(d, want_d[row0:row0 + rows]) and np.array_equal(c, want_c[row0:row0 + rows])


def _matrices(n, positions, links, near=()):
    """diff / compared of n samples in which exactly the pairs of `links` are `links[pair]` apart, every other pair far apart; every pair
    compared everywhere but those of `near`, which map to their compared count."""
    d = np.full((n, n), 1000, np.uint32)
    c = np.full((n, n), positions, np.uint32)
    np.fill_diagonal(d, 0)
    for (i, j), v in links.items():
        d[i, j] = d[j, i] = v
    for (i, j), v in near:
        c[i, j] = c[j, i] = v
    return d, c


@pytest.mark.parametrize("block_rows", [0, 1, 2])
def test_clusterer_on_a_crafted_graph(block_rows):
    positions = 1000
    # samples 0-1-2: a chain, 0-2 over T but joined through 1; 3-4: under T, compared one short of B x positions; 5-6: exactly at both
    # bounds; 7: alone
    d, c = _matrices(8, positions, {(0, 1): 3, (1, 2): 2, (0, 2): 5, (3, 4): 0, (5, 6): 3}, near=[((3, 4), 899), ((5, 6), 900)])
    want = cohort_ref.clusters(d, c, positions, 3, 0.9)
    assert want == ([1, 1, 1, 2, 3, 4, 4, 5], [3, 3, 3, 1, 1, 2, 2, 1])
    cl, size, n_clusters, largest = hostlib.cohort_clusters(d, c, positions, 3, 0.9, block_rows)
    assert (cl.tolist(), size.tolist()) == want and (n_clusters, largest) == (5, 3)
    # B = 0: compared does not matter, 3-4 join; B = 1: only pairs compared everywhere, 5-6 part
    for b, expect in ((0.0, [1, 1, 1, 2, 2, 3, 3, 4]), (1.0, [1, 1, 1, 2, 3, 4, 5, 6])):
        want = cohort_ref.clusters(d, c, positions, 3, b)
        assert want[0] == expect
        cl, size, _, _ = hostlib.cohort_clusters(d, c, positions, 3, b, block_rows)
        assert (cl.tolist(), size.tolist()) == want
    # T = 0: identical pairs only (3-4 are 0 apart but compared too little; at B = 0 they join)
    for b, expect in ((0.9, [1, 2, 3, 4, 5, 6, 7, 8]), (0.0, [1, 2, 3, 4, 4, 5, 6, 7])):
        want = cohort_ref.clusters(d, c, positions, 0, b)
        assert want[0] == expect
        cl, size, _, _ = hostlib.cohort_clusters(d, c, positions, 0, b, block_rows)
        assert (cl.tolist(), size.tolist()) == want


def test_clusterer_on_a_cohort():
    a = cohort_ref.cohort(65, 4999, 3)
    d, c = cohort_ref.distances(a)
    for t, b in ((0, 0.9), (3, 0.9), (8, 0.5), (5000, 0.0)):
        want = cohort_ref.clusters(d, c, 4999, t, b)
        cl, size, n_clusters, largest = hostlib.cohort_clusters(d, c, 4999, t, b, 7)
        assert (cl.tolist(), size.tolist()) == want and n_clusters == max(want[0]) and largest == max(want[1])


def test_writers_equal_the_restatement(tmp_path):
    n, positions = 7, 129
    a = cohort_ref.cohort(n, positions, 11)
    d, c = hostlib.cohort_distances(a)
    names = ["s%d_x" % i for i in range(n)]
    for m, compared, name in ((d, False, "g.distances.tsv"), (c, True, "g.compared.tsv")):
        p = str(tmp_path / name)
        hostlib.write_cohort_matrix_tsv(p, names, m, compared=compared)
        assert open(p, "rb").read() == cohort_ref.matrix_text(names, m)
    for t, b in ((3, 0.9), (0, 0.25), (12, 1.0), (2, 1.0 / 3)):
        number, size = cohort_ref.clusters(d, c, positions, t, b)
        p = str(tmp_path / "g.clusters.tsv")
        hostlib.write_cohort_clusters_tsv(p, names, number, size, t, b)
        assert open(p, "rb").read() == cohort_ref.clusters_text(names, number, size, t, b)
    with pytest.raises(RuntimeError):
        hostlib.write_cohort_matrix_tsv(str(tmp_path / "no_such_dir" / "x.tsv"), names, d)


def test_cli_argument_errors(golden_dir, tmp_path):
    """Each flag without its parent, and the values out of range: reported before any device is touched."""
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    head = ["call", "-d", os.path.join(golden_dir, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")]
    for extra, msg in ((["--distances"], "--distances needs --consensus"),
                       (["--consensus", "--clusters", "3"], "--clusters needs --distances"),
                       (["--consensus", "--distances", "--cluster-min-breadth", "0.5"], "--cluster-min-breadth needs --clusters"),
                       (["--consensus", "--distances", "--clusters", "-1"], "--clusters must be at least 0, got -1"),
                       (["--consensus", "--distances", "--clusters", "3", "--cluster-min-breadth", "1.5"], "--cluster-min-breadth must be between 0 and 1, got 1.5"),
                       (["--consensus", "--distances", "--clusters", "3", "--cluster-min-breadth", "-0.1"], "--cluster-min-breadth must be between 0 and 1")):
        r = subprocess.run([BRONKO] + head + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout and msg in r.stdout, (extra, r.stdout)
        assert "no HIP device" not in r.stdout and not os.path.exists(str(tmp_path / "o"))
    r = subprocess.run([BRONKO] + head + ["--consensus", "--distances", "--clusters"], capture_output=True, text=True)
    assert r.returncode == 2 and "a value is required for '--clusters'" in r.stderr
    r = subprocess.run([BRONKO, "--help"], capture_output=True, text=True)
    for flag in ("--distances", "--clusters T", "--cluster-min-breadth B"):
        assert flag in r.stderr
