"""The read-pileup rule of `bronko call --read-pileup`, restated in plain Python (include/bronko_hip.h bk_sample_read_pileup, DESIGN.md
section U).

The naive loop, written from the rule and not from the C++ or the kernels: for each row, for each of its cells, one increment.  No
difference array, no prefix sum -- it shares no trick with the host twin (bh_read_pileup_count) or the engine (read_pileup_count_kernel,
read_pileup_finish_kernel), which are held against it.  Rows are linkage_ref's: (cell0, n, strand, ((offset, base), ...)).  The
result is an (n_cells, 12) array: per cell fwd[ACGT], rev[ACGT], near[ACGT].
"""
from __future__ import annotations

import numpy as np

from tests.indels_ref import Genome

MAX_END = 255
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
HEADER = ["reference", "index", "ref", "A", "C", "G", "T", "a", "c", "g", "t", "near_A", "near_C", "near_G", "near_T"]


def read_pileup(g: Genome, rows, E: int = 10) -> np.ndarray:
    assert 0 <= E <= MAX_END
    out = [[0] * 12 for _ in range(g.cells)]
    for cell0, n, strand, mm in rows:
        assert 0 <= cell0 and cell0 + n <= g.cells and n >= 1 and strand in (0, 1)
        subs = dict(mm)
        assert len(subs) == len(mm) and all(0 <= off < n for off in subs)
        end = cell0 + n
        for c in range(cell0, end):
            b = subs.get(c - cell0)
            if b is None:
                b = _CODE[g.text[c]]                               # (placement: the reference's letter under a row is one of ACGT)
            out[c][4 * strand + b] += 1
            if min(c - cell0, end - 1 - c) < E:
                out[c][8 + b] += 1
    return np.array(out, np.int64).reshape(g.cells, 12).astype(np.uint32)


def scaled(counts, times: int) -> np.ndarray:
    return (np.asarray(counts, np.int64) * times).astype(np.uint32)


def summary(counts, rows):
    """(covered, bases) as bk_read_pileup_summary gives them; bases must be the sum of the rows' lengths"""
    depth = np.asarray(counts, np.int64)[:, :8].sum(axis=1)
    assert int(depth.sum()) == sum(r[1] for r in rows)
    return int((depth > 0).sum()), int(depth.sum())


def tsv_text(names, seqs, counts, M: int = 8, E: int = 10) -> str:
    """OUT/<stem>.read_pileup.tsv: names and letters of the genome file's sequences as the index holds them (the letter is printed as
    it is), counts of all their positions in order."""
    out = ["##read_pileup_max_mismatches=%d" % M, "##read_pileup_end=%d" % E, "\t".join(HEADER)]
    cell = 0
    for name, s in zip(names, seqs):
        for i, letter in enumerate(s):
            out.append("\t".join([name, str(i + 1), letter] + [str(int(v)) for v in counts[cell]]))
            cell += 1
    assert cell == len(counts)
    return "".join(line + "\n" for line in out)
