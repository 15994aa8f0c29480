"""--contamination without a GPU: the host twins of the mask kernel and of the explained kernel, the scanner and the three writers
(bronko_amd/host/cohort.cpp) against the plain-numpy restatement (tests/contamination_ref.py), and the argument checks of the five
options."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import hostlib
from tests import cohort_ref, consensus_ref, contamination_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
NONE = 0xffffffff

POSITIONS = (1, 63, 64, 65, 127, 128, 129, 4999)
SAMPLES = (1, 2, 3, 63, 64, 65, 130)
CASES = sorted(set([(n, 129) for n in SAMPLES] + [(5, p) for p in POSITIONS] + [(65, 4999)]))
# (R, F) with exact-threshold cells in the crafted pileups: counts of 10 and 9, a quarter and a half of a depth, F = 0 and F = 1
MINOR_PARAMS = [(10, 0.03), (10, 0.0), (1, 0.25), (1, 0.5), (1, 1.0), (20, 0.25), (300, 0.5)]


@pytest.mark.parametrize("n,positions", CASES)
def test_explained_twin_equals_the_restatement(n, positions):
    a, m = contamination_ref.cohort(n, positions, 1000 * n + positions)
    want, want_sites = contamination_ref.explained(a, m)
    diff, _ = cohort_ref.distances(a)
    for threads in (1, 16):
        ex, sites = hostlib.cohort_explained(a, m, threads=threads)
        assert np.array_equal(ex, want) and np.array_equal(sites, want_sites)
    assert not want.diagonal().any() and (want <= diff).all() and (want <= want_sites[:, None]).all()
    if n >= 5:                                                   # mask 15 against the sample that differs everywhere
        assert want[2, 3] == diff[2, 3] == positions == want_sites[2]
    if n >= 2:                                                   # mask 0 everywhere
        assert not want[n - 1].any() and want_sites[n - 1] == 0
    if n >= 4:                                                   # minor alleles that are exactly another sample's differences
        assert want[0, n - 2] == diff[0, n - 2] == want_sites[0]
    if n >= 3:                                                   # the all-N sample: nothing as a recipient, nothing as a source
        assert not want[1].any() and not want[:, 1].any() and want_sites[1] == 0
    if n >= 5 and positions >= 63:                               # not symmetric: random masks on the other side of the planted pair
        assert want[3, 2] < want[2, 3]
    for row0, rows in ((0, 1), (n - 1, 1), (n // 2, n - n // 2)):
        ex, sites = hostlib.cohort_explained(a, m, row0, rows)
        assert np.array_equal(ex, want[row0:row0 + rows]) and np.array_equal(sites, want_sites[row0:row0 + rows])


def test_the_upper_four_bits_of_a_mask_are_ignored():
    a, m = contamination_ref.cohort(65, 129, 11)
    want = contamination_ref.explained(a, m & 15)
    for got in (contamination_ref.explained(a, m), hostlib.cohort_explained(a, m)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (m >> 4).any()


def test_mask_twin_on_the_crafted_pileups():
    n = 0
    for case in consensus_ref.crafted_cases():
        for cell0, length in case.layout.seqs:
            fwd, rev = case.fwd[cell0 * 4:(cell0 + length) * 4], case.rev[cell0 * 4:(cell0 + length) * 4]
            for r, f in MINOR_PARAMS:
                want, tallies = contamination_ref.present_masks(fwd, rev, r, f)
                got, got_t = hostlib.minor_mask(fwd, rev, r, f)
                assert np.array_equal(got, want) and got_t == tuple(tallies[k] for k in contamination_ref.TALLIES), (case.name, cell0, r, f)
                n += length
    assert n > 7 * 10000


def test_mask_rule_at_its_thresholds():
    def mask(counts, r, f):
        fwd = np.array(counts, np.uint64)
        m, t = contamination_ref.present_masks(fwd, np.zeros(4, np.uint64), r, f)
        assert np.array_equal(hostlib.minor_mask(fwd, np.zeros(4, np.uint64), r, f)[0], m)
        return int(m[0])
    assert mask([90, 10, 9, 0], 10, 0.0) == 3                    # tot == R is present, tot == R - 1 is not
    assert mask([75, 25, 0, 0], 1, 0.25) == 3                    # tot == F x depth is present
    assert mask([76, 24, 0, 0], 1, 0.25) == 1
    assert mask([50, 50, 0, 0], 1, 0.5) == 3
    assert mask([51, 49, 0, 0], 1, 0.5) == 1
    assert mask([5, 3, 1, 0], 1, 0.0) == 7                       # F = 0: every base with R reads
    assert mask([7, 0, 0, 0], 1, 1.0) == 1 and mask([6, 1, 0, 0], 1, 1.0) == 0   # F = 1: a base alone
    assert mask([0, 0, 0, 0], 1, 0.0) == 0                       # no depth: R >= 1 keeps every bit out


def _matrices(n, positions, seed):
    a, m = contamination_ref.cohort(n, positions, seed)
    d, c = cohort_ref.distances(a)
    ex, sites = contamination_ref.explained(a, m)
    return d, c, ex, sites


def _check_scan(d, c, ex, s, p, block_rows):
    flagged, best, counts, recipients, largest = hostlib.contamination_scan(d, c, ex, s, p, block_rows)
    want_f, want_b, want_c = contamination_ref.scan(d, ex, s, p)
    assert [(int(r[0]), int(r[1])) for r in flagged] == want_f
    for r in flagged:
        i, j = int(r[0]), int(r[1])
        assert (int(r[2]), int(r[3]), int(r[4])) == (int(d[i, j]), int(c[i, j]), int(ex[i, j]))
    assert [None if int(b[0]) == NONE else int(b[0]) for b in best] == want_b
    for i, j in enumerate(want_b):
        if j is not None:
            assert (int(best[i][1]), int(best[i][2])) == (int(ex[i, j]), int(d[i, j]))
    assert counts.tolist() == want_c and recipients == sum(1 for v in want_c if v)
    off = ex.copy()
    np.fill_diagonal(off, 0)
    assert largest == int(off.max())
    return want_f


@pytest.mark.parametrize("block_rows", [0, 1, 2])
def test_scanner_equals_the_restatement(block_rows):
    for n, positions in ((1, 129), (2, 129), (5, 129), (65, 129)):
        d, c, ex, _ = _matrices(n, positions, 1000 * n + positions)
        for s, p in ((1, 0.0), (3, 0.75), (1, 1.0), (50, 0.5)):
            _check_scan(d, c, ex, s, p, block_rows)


@pytest.mark.parametrize("block_rows", [0, 1, 2])
def test_scanner_thresholds_and_ties(block_rows):
    z = np.zeros((4, 4), np.uint32)
    # recipient 0: source 1 misses S = 3 by one; source 2 misses P x diff = 0.75 x 8 = 6 by one; source 3 meets both exactly
    d, ex = z.copy(), z.copy()
    d[0] = [0, 2, 8, 8]
    ex[0] = [0, 2, 5, 6]
    c = d + 100
    assert _check_scan(d, c, ex, 3, 0.75, block_rows) == [(0, 3)]
    assert _check_scan(d, c, ex, 3, 0.0, block_rows) == [(0, 2), (0, 3)]     # P = 0: S alone decides
    assert _check_scan(d, c, ex, 2, 1.0, block_rows) == [(0, 1)]             # P = 1: every difference is explained
    assert _check_scan(d, c, ex, 2, 0.0, block_rows) == [(0, 1), (0, 2), (0, 3)]
    # best source: the largest explained; ties go to the smaller diff, then to the earlier sample
    d, ex = z.copy(), z.copy()
    ex[0] = [0, 4, 4, 4]
    d[0] = [0, 9, 6, 6]
    ex[1] = [4, 0, 4, 5]
    d[1] = [7, 0, 7, 30]
    ex[2] = [3, 3, 0, 0]
    d[2] = [5, 5, 0, 0]
    _, best, _, _, largest = hostlib.contamination_scan(d, d + 1, ex, 3, 0.75, block_rows)
    assert [int(b[0]) for b in best] == [2, 3, 0, NONE] and largest == 5
    assert contamination_ref.scan(d, ex, 3, 0.75)[1] == [2, 3, 0, None]


def test_writers_byte_for_byte(tmp_path):
    for n, positions, block_rows in ((5, 129, 0), (65, 129, 2), (2, 63, 1), (1, 64, 0)):
        d, c, ex, sites = _matrices(n, positions, 1000 * n + positions)
        names = ["s%d" % i for i in range(n)]
        p = str(tmp_path / "x.tsv")
        hostlib.write_cohort_explained_tsv(p, names, ex)
        assert open(p, "rb").read() == contamination_ref.explained_text(names, ex)
        for r, f, s, share in ((10, 0.03, 3, 0.75), (1, 0.0, 1, 0.0), (7, 0.125, 2, 1.0)):
            hostlib.write_contamination_tsv(p, names, d, c, ex, sites, r, f, s, share, block_rows=block_rows)
            want = contamination_ref.contamination_text(names, d, c, ex, sites, r, f, s, share)
            assert open(p, "rb").read() == want
            hostlib.write_contamination_tsv(p, names, d, c, ex, sites, r, f, s, share, mixture=True, block_rows=block_rows)
            assert open(p, "rb").read() == contamination_ref.mixture_text(names, d, ex, sites, r, f, s, share)
        if n == 65:
            assert want.count(b"\n") > 6                         # (there are flagged lines to compare)
    # the ratios are truncated, not rounded: 2 / 3 = 0.6666, 5 / 6 = 0.8333, 1 / 1 = 1.0000
    d = np.array([[0, 3], [6, 0]], np.uint32)
    ex = np.array([[0, 2], [5, 0]], np.uint32)
    hostlib.write_contamination_tsv(p, ["a", "b"], d, d + 9, ex, [2, 7], 10, 0.03, 1, 0.5)
    assert open(p, "rb").read().endswith(b"a\tb\t3\t12\t2\t0.6666\t2\t1.0000\nb\ta\t6\t15\t5\t0.8333\t7\t0.7142\n")
    with pytest.raises(RuntimeError):
        hostlib.write_cohort_explained_tsv(str(tmp_path / "no_such_dir" / "x.tsv"), ["a", "b"], ex)


def test_cli_argument_errors(golden_dir, tmp_path):
    """Each of the five options without its parent, and the values out of range: reported before any device is touched."""
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    head = ["call", "-d", os.path.join(golden_dir, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")]
    on = ["--consensus", "--distances", "--contamination"]
    for extra, msg in ((["--consensus", "--contamination"], "--contamination needs --distances"),
                       (["--consensus", "--distances", "--minor-min-reads", "5"], "--minor-min-reads needs --contamination"),
                       (["--consensus", "--distances", "--minor-min-freq", "0.1"], "--minor-min-freq needs --contamination"),
                       (["--consensus", "--distances", "--contamination-min-sites", "2"], "--contamination-min-sites needs --contamination"),
                       (["--consensus", "--distances", "--contamination-min-share", "0.5"], "--contamination-min-share needs --contamination"),
                       (on + ["--minor-min-reads", "0"], "--minor-min-reads must be at least 1, got 0"),
                       (on + ["--minor-min-freq", "1.5"], "--minor-min-freq must be between 0 and 1, got 1.5"),
                       (on + ["--minor-min-freq", "-0.1"], "--minor-min-freq must be between 0 and 1, got -0.1"),
                       (on + ["--contamination-min-sites", "0"], "--contamination-min-sites must be at least 1, got 0"),
                       (on + ["--contamination-min-share", "1.1"], "--contamination-min-share must be between 0 and 1, got 1.1"),
                       (on + ["--contamination-min-share", "-0.5"], "--contamination-min-share must be between 0 and 1, got -0.5")):
        r = subprocess.run([BRONKO] + head + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout and msg in r.stdout, (extra, r.stdout)
        assert "no HIP device" not in r.stdout and not os.path.exists(str(tmp_path / "o"))
    r = subprocess.run([BRONKO] + head + on + ["--minor-min-reads"], capture_output=True, text=True)
    assert r.returncode == 2 and "a value is required for '--minor-min-reads'" in r.stderr
    r = subprocess.run([BRONKO, "--help"], capture_output=True, text=True)
    for flag in ("--contamination ", "--minor-min-reads R", "--minor-min-freq F", "--contamination-min-sites S", "--contamination-min-share P"):
        assert flag in r.stderr
