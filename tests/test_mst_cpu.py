"""--mst without a GPU: the host twin of bk_cohort_mst (Prim, bronko_amd/host/cohort.cpp), the rooting and the writer against the
restatement (tests/mst_ref.py: Kruskal and a plain Boruvka), the forest's relation to --clusters, and the flags' argument checks."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import hostlib
from tests import cohort_ref, mst_cases, mst_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")

SAMPLES = (1, 2, 3, 63, 64, 65, 130)
POSITIONS = (129, 700, 4999)


def _tuples(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("kind", mst_cases.KINDS)
def test_host_twin_equals_the_restatement(tmp_path, kind, n, positions):
    a, d, c = mst_cases.case(kind, n, positions)
    names = ["s%d_x" % i for i in range(n)]
    for need, breadth in zip(mst_cases.needs(positions), (0.0, 0.5, 0.9)):
        assert hostlib.cohort_min_compared(breadth, positions) == need
        want_edges, want_near, _ = mst_cases.expected(kind, n, positions, need)
        for threads in (1, 16):
            edges, near = hostlib.cohort_mst(a, need, threads=threads)
            assert _tuples(edges) == want_edges and _tuples(near) == want_near, (need, threads)
        got = hostlib.cohort_root_forest(n, edges)
        want = mst_ref.root(n, want_edges)
        assert [g.tolist() for g in got[:5]] == [list(w) for w in want]
        assert got[5] == max(want[3]) and got[6] == max(want[4]) and got[7] == max([e[2] for e in want_edges], default=0)
        p = str(tmp_path / ("g%d.mst.tsv" % need))
        hostlib.write_cohort_mst_tsv(p, names, edges, near, breadth, need)
        assert open(p, "rb").read() == mst_ref.mst_text(names, want_edges, want_near, breadth, need)


def test_the_cases_are_what_they_are_meant_to_be():
    """The ruler chain needs about log2 n rounds, the related cohort's edges tie, the clonal cohort falls apart at a high bound."""
    for positions in (700, 4999):
        for breadth in (0.5, 0.97):
            need = mst_ref.min_compared(breadth, positions)
            assert [mst_ref.boruvka(*mst_cases.case("ruler", n, positions)[1:], need)[1] for n in (64, 65, 130)] == [6, 6, 7]
    edges, _, rounds = mst_cases.expected("related", 63, 129, 0)
    assert rounds == 2 and len(edges) - len(set(e[2] for e in edges)) > 50
    _, d, c = mst_cases.case("clonal", 130, 4999)
    need = mst_ref.min_compared(0.97, 4999)
    comp = mst_ref.components_of(130, mst_ref.kruskal(d, c, need))
    near = mst_ref.nearest(d, c, need)
    assert max(comp) > 20 and sum(1 for x in near if x[0] == mst_ref.NONE) > 10


@pytest.mark.parametrize("kind,n,positions", [("related", 65, 4999), ("clonal", 130, 700), ("clonal", 64, 4999), ("ruler", 65, 700), ("related", 130, 129)])
def test_the_forest_cut_at_t_is_the_clusters_of_t(kind, n, positions):
    """For any T and any min_compared >= 1 the forest's edges with diff <= T connect exactly the clusters of --clusters T with the
    same breadth bound."""
    a, d, c = mst_cases.case(kind, n, positions)
    for breadth in (0.5, 0.9, 0.97):
        need = mst_ref.min_compared(breadth, positions)
        assert need >= 1
        edges, _ = hostlib.cohort_mst(a, need, threads=4)
        for t in (0, 3, 1000):
            number, _ = cohort_ref.clusters(d, c, positions, t, breadth)
            assert mst_ref.components_of(n, [e for e in _tuples(edges) if e[2] <= t]) == number, (breadth, t)


def test_compared_one_short_of_the_bound():
    positions = 100
    a = np.full((3, positions), ord("A"), np.uint8)
    a[1, :11] = ord("N")                                         # 0-1 compare 89 positions, 0-2 compare 90, 1-2 compare 79
    a[2, 20:30] = ord("N")
    a[2, 50] = ord("C")
    edges, near = hostlib.cohort_mst(a, 90)
    assert _tuples(edges) == [(0, 2, 1, 90)]
    assert _tuples(near) == [(2, 1, 90), (mst_ref.NONE, 0, 0), (0, 1, 90)]
    edges, near = hostlib.cohort_mst(a, 89)
    assert _tuples(edges) == [(0, 1, 0, 89), (0, 2, 1, 90)]
    assert _tuples(near) == [(1, 0, 89), (0, 0, 89), (0, 1, 90)]
    d, c = cohort_ref.distances(a)
    for need in (89, 90):
        assert _tuples(hostlib.cohort_mst(a, need)[0]) == mst_ref.kruskal(d, c, need)


def test_a_sample_without_a_base_stays_alone_at_min_compared_0():
    a, d, c = mst_cases.case("related", 65, 129)                 # (sample 1 is all N)
    assert not c[1].any()
    edges, near = hostlib.cohort_mst(a, 0)
    assert all(1 not in e[:2] for e in _tuples(edges)) and tuple(near[1]) == (mst_ref.NONE, 0, 0)
    assert all(x[0] != 1 for x in _tuples(near))
    forest = hostlib.cohort_root_forest(65, edges)
    assert forest[0][1] == mst_ref.NONE and forest[4][1] == 1    # a root, a component of one


def test_root_forest_refuses_what_is_no_forest():
    with pytest.raises(RuntimeError):
        hostlib.cohort_root_forest(3, [(0, 1, 1, 9), (1, 2, 1, 9), (0, 2, 1, 9)])
    with pytest.raises(RuntimeError):
        hostlib.cohort_root_forest(3, [(1, 3, 1, 9)])


def test_cli_argument_errors(golden_dir, tmp_path):
    """Each flag without its parent, and the values out of range: reported, with the value, before any device is touched."""
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    head = ["call", "-d", os.path.join(golden_dir, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")]
    for extra, msg in ((["--consensus", "--mst"], "--mst needs --distances"),
                       (["--consensus", "--distances", "--mst-min-breadth", "0.5"], "--mst-min-breadth needs --mst"),
                       (["--consensus", "--distances", "--mst", "--mst-min-breadth", "1.5"], "--mst-min-breadth must be between 0 and 1, got 1.5"),
                       (["--consensus", "--distances", "--mst", "--mst-min-breadth", "-0.1"], "--mst-min-breadth must be between 0 and 1, got -0.1")):
        r = subprocess.run([BRONKO] + head + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout and msg in r.stdout, (extra, r.stdout)
        assert "no HIP device" not in r.stdout and not os.path.exists(str(tmp_path / "o"))
    r = subprocess.run([BRONKO] + head + ["--consensus", "--distances", "--mst", "--mst-min-breadth"], capture_output=True, text=True)
    assert r.returncode == 2 and "a value is required for '--mst-min-breadth'" in r.stderr
    r = subprocess.run([BRONKO, "--help"], capture_output=True, text=True)
    for flag in ("[--mst]", "--mst-min-breadth B", "<genome>.mst.tsv"):
        assert flag in r.stderr
