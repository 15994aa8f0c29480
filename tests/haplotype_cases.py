"""Inputs of the haplotype tests (tests/test_haplotypes_cpu.py, tests/test_gpu_haplotypes.py): crafted regions on indel_cases' crafted
two-sequence genome to go with codon_cases' crafted records (and a few records more), and window tilings of HPV16 for codon_cases'
planted sample.  What the rule makes of them is haplotypes_ref's business."""
from __future__ import annotations

import functools

from tests import codon_cases, haplotypes_ref, indel_cases, indels_ref
from tests.indel_cases import mut_read
from tests.linkage_cases import N_LEN, START


def crafted_cases(k: int):
    """codon_cases.crafted_cases(k) and records that agree with one of them inside a region and differ outside it."""
    (_, a), _ = indel_cases.crafted_genome(k)
    extra = [("apart_2_and_90", mut_read(a, START, N_LEN, subs=(70, 72, 90))),     # apart_2 inside [START + 60, START + 80)
             ("apart_2_and_5", mut_read(a, START, N_LEN, subs=(5, 70, 72))),
             ("apart_2_longer", mut_read(a, START - 7, 160, subs=(77, 79)))]         # the same cells from another first cell, another length
    out = codon_cases.crafted_cases(k)
    for label, read in extra:
        out.append((label, read))
        out.append((label + "/rc", indels_ref.revcomp(read)))
    return out


def crafted_regions(k: int):
    """[(cell0, len)] on indel_cases.crafted_genome(k).  The records at START cover [START, START + 150); mm_8 has its eight
    substitutions at START + 40 + 9 t."""
    (_, a), (_, b) = indel_cases.crafted_genome(k)
    first_b, end = len(a), START + N_LEN
    return [(START, N_LEN),                                # from a record's first cell to its last
            (START - 1, N_LEN + 1), (START, N_LEN + 1),    # one cell further on either side: only the longer records span these
            (START, 10), (end - 10, 10),                   # begins at the first cell, ends at the last
            (START - 1, 10), (end - 9, 10),                # ... one cell further out
            (START + 40, 64),                              # mm_8: a substitution on the first cell and on the last, all eight inside
            (START + 41, 62),                              # ... both just outside
            (START + 60, 20), (START + 60, 20),            # apart_2 and the records that differ from it outside; the same region again
            (START + 65, 10), (START + 70, 1), (START + 72, 1), (START + 71, 1),   # nested; single cells
            (START + 10, 100), (START + 50, 100),          # overlapping
            (1290, 40),                                    # over the stretch of N [1300, 1320): no row
            (1250, 50),                                    # ends at the last cell in front of it
            (len(a) - 30, 30),                             # ends at the first sequence's last cell
            (first_b + 100, 60), (first_b + 105, 10), (first_b, 30),   # the second sequence
            (START - 300, 260)]                            # in front of the records at START and longer than any record


HOT_START = 1990


def hot_reads(g_text: str, n: int = 2000):
    """n reads of one haplotype from one first cell, along and against the reference in turn: every row is the same but for its strand"""
    read = mut_read(g_text, HOT_START, N_LEN, subs=(10, 12, 73))
    return [read, indels_ref.revcomp(read)] * (n // 2)


HOT_REGIONS = [(HOT_START, N_LEN), (HOT_START + 5, 30), (HOT_START + 13, 50), (HOT_START + 70, 10), (HOT_START + 5, 30)]


class Planted(codon_cases.Planted):
    """codon_cases' planted sample (HPV16, k = 21, 2,000 reads) under two tilings, and what the restatement makes of them (computed
    once, shared, left unchanged)."""

    def __init__(self):
        super().__init__(21)
        self.wins_a = haplotypes_ref.windows(self.g, 100, 50)
        self.wins_b = haplotypes_ref.windows(self.g, 30, 10)
        self.regs_a, self.regs_b = haplotypes_ref.regions_of(self.wins_a), haplotypes_ref.regions_of(self.wins_b)
        self.table_a = haplotypes_ref.hap_count(self.g, self.rows, self.regs_a)
        self.table_b = haplotypes_ref.hap_count(self.g, self.rows, self.regs_b)
        self.placed = self.tallies["placed"]
        na, nb = len(self.table_a[2]), len(self.table_b[2])
        assert (self.placed, len(self.wins_a), na, len(self.wins_b), nb) == (1955, 157, 752, 788, 2948), (self.placed, len(self.wins_a), na, len(self.wins_b), nb)
        # the first tiling fits a table of 2^10 slots, tightly (load 0.73: long probes); the second overflows it and fits 2^12
        assert 0.7 * (1 << 10) < na <= (1 << 10) < nb <= (1 << 12)
        assert sum(self.table_a[0]) > 1000 and max(c for _, c, _ in self.table_a[2]) > 20   # (some 47 reads span a window of 100, most of them of haplotype 1)


@functools.lru_cache(maxsize=None)
def planted() -> Planted:
    return Planted()
