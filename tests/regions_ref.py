"""The per-region depth report of `bronko call --regions / --region-window` (bk_sample_region_depths) restated in plain Python, and
the cases the host twin and the device kernel are held against (tests only; shared by tests/test_regions_cpu.py and
tests/test_gpu_regions.py).

The rule (include/bronko_hip.h): depth[p] = the four bases' forward + reverse depths; per region [start, end) of one sequence, with
L = end - start: sum, min, max, median = sorted(d)[(L - 1) // 2] (the lower median), covered = positions with depth >= D.  A region
is full when covered == L, empty when covered == 0, partial otherwise.  The mean is printed from integers: m = 100 * sum // L as
m // 100 "." two digits of m % 100.  Python integers throughout: nothing rounds, nothing wraps.

A region here is (file_id, seq, start, end, name); a row is (sum, min, max, median, covered).
"""
import random

import numpy as np

from tests import pileup_cases

LDS = 2048                                   # positions of a region the kernel stages in LDS (bk_kernels.h kRegionLdsDepths)
SHAPES = [1, 2, 3, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1]
DEPTHS = [1, 10, 300]                        # the D every case is checked at
HEADER = "chrom\tstart\tend\tname\tlength\tmean\tmin\tmedian\tmax\tcovered\n"


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def cell_depths(fwd, rev):
    """depth of every cell, as Python integers"""
    f = np.asarray(fwd, np.uint64).reshape(-1, 4)
    r = np.asarray(rev, np.uint64).reshape(-1, 4)
    return [sum(int(v) for v in f[c]) + sum(int(v) for v in r[c]) for c in range(len(f))]


def region_row(d, min_depth):
    """(sum, min, max, median, covered) of a region's depths"""
    L = len(d)
    assert L >= 1 and min_depth >= 1
    return (sum(d), min(d), max(d), sorted(d)[(L - 1) // 2], sum(1 for v in d if v >= min_depth))


def report(file_seqs, depths, regions, file_id, min_depth):
    """(rows, (full, partial, empty)) of the regions of `file_id`, in order.  file_seqs[f] = [(first cell, length)] of file f's
    sequences, depths = cell_depths() of all cells."""
    rows, full, partial, empty = [], 0, 0, 0
    for r in regions:
        if r[0] != file_id:
            continue
        cell0, length = file_seqs[r[0]][r[1]]
        assert 0 <= r[2] < r[3] <= length
        row = region_row(depths[cell0 + r[2]:cell0 + r[3]], min_depth)
        rows.append(row)
        L = r[3] - r[2]
        if row[4] == L:
            full += 1
        elif row[4] == 0:
            empty += 1
        else:
            partial += 1
    return rows, (full, partial, empty)


def mean_text(total, L):
    m = 100 * total // L
    return "%d.%02d" % (m // 100, m % 100)


def tsv_text(min_depth, chroms, regions, file_id, rows):
    """OUT/<stem>.regions.tsv as bytes; chroms[seq] = the CHROM token of the selected file's sequences"""
    out = ["##min_depth=%d\n" % min_depth, HEADER]
    mine = [r for r in regions if r[0] == file_id]
    assert len(mine) == len(rows)
    for r, (total, lo, hi, med, cov) in zip(mine, rows):
        L = r[3] - r[2]
        out.append("%s\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%d\n" % (chroms[r[1]], r[2], r[3], r[4] if len(r) > 4 else ".", L, mean_text(total, L), lo, med, hi, cov))
    return "".join(out).encode()


def window_regions(files_seq_lens, window):
    """--region-window: [iW, min((i + 1)W, len)) over every sequence of every file; files_seq_lens[f] = [length of each sequence]"""
    return [(f, q, s, min(s + window, n), ".") for f, lens in enumerate(files_seq_lens) for q, n in enumerate(lens) for s in range(0, n, window)]


# ---- layouts and depth patterns ----------------------------------------------------------------------------------------------------
_long = []


def layout(name):
    """`lengths` and `multi` of tests/pileup_cases.py (the target behind a decoy's cells; lengths 1..1100), and `long`: sequences
    of 3100, 700 and 1 positions behind a decoy, the first one longer than the kernel's LDS buffer"""
    if name != "long":
        return pileup_cases.layout(name)
    if not _long:
        rng = random.Random(21)
        files = [("decoy", [("d1", pileup_cases.random_sequence(rng, 90))]),
                 ("long", [("long_s%d" % j, pileup_cases.random_sequence(rng, n)) for j, n in enumerate([3100, 700, 1])])]
        _long.append(pileup_cases.Layout("long", files, 1))
    return _long[0]


def _spread(case, cell, depth, rng, strands=(0, 1)):
    """`depth` over the eight counts of a cell, at random (only the given strands)"""
    arr = (case.fwd, case.rev)
    for b in range(4):
        case.fwd[cell * 4 + b] = case.rev[cell * 4 + b] = 0
    left = depth
    slots = [(s, b) for s in strands for b in range(4)]
    rng.shuffle(slots)
    for j, (s, b) in enumerate(slots[:3]):
        part = left if j == 2 else rng.randrange(0, left + 1)
        arr[s][cell * 4 + b] += np.uint64(part)
        left -= part


PATTERNS = ["equal", "zero", "rising", "falling", "alternate", "halves", "outlier", "thresholds", "forward_only", "random"]


def _depth_at(pattern, i, n, rng):
    if pattern == "equal":
        return 37
    if pattern == "zero":
        return 0
    if pattern == "rising":
        return 3 * i
    if pattern == "falling":
        return 3 * (n - i)
    if pattern == "alternate":                   # two values half and half over every even L; the rank sits on the boundary
        return 500 if i % 2 else 5
    if pattern == "halves":                      # ... and as two runs around the sequence's middle
        return 7 if i < n // 2 else 400
    if pattern == "outlier":
        return 1 + i % 9
    if pattern == "thresholds":                  # D - 1, D, D + 1 of every D
        return [9, 10, 11, 299, 300, 301, 0, 1, 2][i % 9]
    return rng.choice([0, 0, 1, 9, 10, 11, 299, 300, 301, rng.randrange(0, 5000), rng.randrange(0, 1 << 20)])


def pattern_case(lay, pattern, seed=0):
    """A pileup of the layout's target after the pattern; the decoy's cells hold other numbers, which a wrong offset would read."""
    rng = random.Random("%s/%s/%d" % (lay.name, pattern, seed))
    c = pileup_cases.Case("regions_%s_%s" % (lay.name, pattern), "regions", lay, pileup_cases.Params(**pileup_cases.LOOSE))
    for f, seqs in enumerate(lay.file_seqs):
        for cell0, n in seqs:
            for i in range(n):
                if f != lay.target:
                    _spread(c, cell0 + i, 100000 + 13 * i, rng)
                else:
                    _spread(c, cell0 + i, _depth_at(pattern, i, n, rng), rng, strands=(0,) if pattern == "forward_only" else (0, 1))
    if pattern == "outlier":                     # one position in ~150 with 10^12 on each strand
        for cell0, n in lay.seqs:
            for i in range(n // 2, n, 151):
                c.fwd[(cell0 + i) * 4 + 1] = np.uint64(10 ** 12)
                c.rev[(cell0 + i) * 4 + 2] = np.uint64(10 ** 12)
    return c


def shape_regions(lay):
    """The regions every pattern is reported over: every shape of SHAPES at a sequence's first position, at its last and in its
    middle, the whole sequence, adjacent, overlapping, nested and identical ranges, a few of the decoy file in between (another
    file's slice of the table), in no particular order of sequences."""
    out = []
    t = lay.target
    for q, (_, n) in enumerate(lay.seqs):
        out.append((t, q, 0, n, "whole_%d" % q))
        for L in SHAPES:
            if L <= n:
                out.append((t, q, 0, L, "first_%d_%d" % (q, L)))
                out.append((t, q, n - L, n, "."))
                out.append((t, q, (n - L) // 2, (n - L) // 2 + L, "mid_%d_%d" % (q, L)))
        if n >= 8:
            a, b, m = n // 4, n // 2, n // 2 + n // 4
            out += [(t, q, a, b, "adjacent_a"), (t, q, b, m, "adjacent_b"), (t, q, a + 1, m - 1, "overlapping"), (t, q, a + 2, b - 1, "nested"),
                    (t, q, a, b, "identical"), (t, q, n - 1, n, "last"), (t, q, 0, 1, "first")]
        if q % 3 == 1:
            d0 = lay.file_seqs[1 - t][0][1]
            out.append((1 - t, 0, 0, d0, "decoy_whole"))
            out.append((1 - t, 0, d0 // 3, d0 // 2, "decoy_part"))
    rng = random.Random(lay.name)
    rng.shuffle(out)
    return out


def expected(case, regions, min_depth, file_id=None):
    """(rows, tallies) of the case's pileup by the rule; the cells' depths are kept with the case"""
    if getattr(case, "_region_depths", None) is None:
        case._region_depths = cell_depths(case.fwd, case.rev)
    return report(case.layout.file_seqs, case._region_depths, regions, case.layout.target if file_id is None else file_id, min_depth)


def random_regions(lay, rng, count, max_len=3000):
    out = []
    for _ in range(count):
        f = rng.randrange(len(lay.file_seqs))
        q = rng.randrange(len(lay.file_seqs[f]))
        n = lay.file_seqs[f][q][1]
        L = rng.randrange(1, min(n, max_len) + 1)
        s = rng.randrange(0, n - L + 1)
        out.append((f, q, s, s + L, "r%d" % len(out) if rng.random() < 0.7 else "."))
    return out
