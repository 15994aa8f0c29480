"""Inputs of the codon tests (tests/test_codons_cpu.py, tests/test_gpu_codons.py): crafted regions on indel_cases' crafted two-sequence
genome to go with linkage_cases' crafted records (and a few records more), and a sample of reads of HPV16 drawn from two planted
haplotypes that put two and three substitutions into one codon.  What the rule makes of them is codons_ref's business."""
from __future__ import annotations

import random

from tests import codons_ref, indel_cases, indels_ref, linkage_cases, linkage_ref
from tests.indel_cases import mut_read
from tests.linkage_cases import HPV, N_LEN, SAMPLE_P, SAMPLE_SPAN, START


def crafted_cases(k: int):
    """linkage_cases.crafted_cases(k) and records with two and three mismatches in one codon, along and against the reference."""
    (_, a), _ = indel_cases.crafted_genome(k)
    extra = [("triple", mut_read(a, START, N_LEN, subs=(90, 91, 92))),                # one codon of the frame at START, two of the others
             ("pair_and_single", mut_read(a, START, N_LEN, subs=(60, 61, 66))),
             ("first_and_last_codon", mut_read(a, START, N_LEN, subs=(1, 2, 147, 149))),
             ("shifted", mut_read(a, START + 1, N_LEN, subs=(69, 71)))]                # the cells of apart_2 from another first cell
    out = linkage_cases.crafted_cases(k)
    for label, read in extra:
        out.append((label, read))
        out.append((label + "/rc", indels_ref.revcomp(read)))
    return out


def crafted_regions(k: int):
    """[(cell0, n_codons)] on indel_cases.crafted_genome(k).  The records at START cover [START, START + 150)."""
    (_, a), (_, b) = indel_cases.crafted_genome(k)
    first_b, end = len(a), START + N_LEN
    regions = [(START, 50), (START + 1, 50), (START + 2, 49),     # the three frames: offsets 70 and 72 share a codon of the second, 90..92 one of the first
               (START, 10),                                       # begins exactly at a record's first cell
               (end - 30, 10),                                    # ends exactly at its last cell
               (START - 1, 20),                                   # begins one cell in front: the edge codon is not counted
               (end - 29, 10),                                    # ends one cell behind
               (START + 70, 1),                                   # one codon
               (START, 50),                                       # the same region again
               (START + 31, 5),                                   # nested in the first, in another frame
               (1290, 15),                                        # over the stretch of N [1300, 1320)
               (len(a) - 30, 10),                                 # ends at the first sequence's last cell
               (first_b + 100, 40), (first_b + 101, 30), (first_b, 8),   # the second sequence
               (START - 300, 260)]                                # a long one in front that reaches over all of the records at START
    assert START + 70 == START + 1 + 3 * 23 and START + 90 == START + 3 * 30
    return regions


HAP1 = (0, 2, 63, 64, 65, 203, 1500)   # offsets from SAMPLE_P: two substitutions in the codon at SAMPLE_P, three in the one at SAMPLE_P + 63
HAP2 = (30, 100)
SAMPLE_SEED = 1


def sample_reads(g: str, seed: int = SAMPLE_SEED, n_reads: int = 2000, length: int = N_LEN, span=SAMPLE_SPAN):
    """Reads of both strands from `span` of the genome, 70 % from haplotype 1 and 30 % from haplotype 2, 0.5 % of the bases
    substituted (linkage_cases.sample_reads with these haplotypes)."""
    rng = random.Random(seed)
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    haps = []
    for offs in (HAP1, HAP2):
        h = list(g)
        for o in offs:
            h[SAMPLE_P + o] = nxt[h[SAMPLE_P + o]]
        haps.append("".join(h))
    reads = []
    for _ in range(n_reads):
        start = rng.randrange(span[0], span[1] - length)
        out = list(haps[0 if rng.random() < 0.7 else 1][start:start + length])
        for o in range(length):
            if rng.random() < 0.005:
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
        r = "".join(out)
        reads.append(indels_ref.revcomp(r) if rng.random() < 0.5 else r)
    return reads


def alt_triplet(g, cell: int, offsets) -> int:
    """the triplet of the codon at `cell` with the planted substitutions at `offsets` (from the codon's first cell)"""
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    t = [nxt[c] if i in offsets else c for i, c in enumerate(g.text[cell:cell + 3])]
    return sum("ACGT".index(c) << (4 - 2 * i) for i, c in enumerate(t))


class Planted:
    """HPV16 at k = 21, the planted sample and what the restatement makes of it (computed once, shared, left unchanged)."""

    def __init__(self, k: int = 21):
        self.k = k
        self.g = indels_ref.read_fasta(HPV, k)
        self.reads = sample_reads(self.g.text)
        self.rows, self.tallies = linkage_ref.link_rows(self.g, self.reads, 8)
        n = self.g.cells
        self.frames = [(f, (n - f) // 3) for f in range(3)]               # the whole genome in its three frames
        self.counts = codons_ref.codon_count(self.g, self.rows, self.frames)
        # a few genes around the planted cells: both strands, another frame, nested
        self.genes = [(SAMPLE_P, 100, 0, SAMPLE_P, "+", "geneA"), (SAMPLE_P - 60, 150, 0, SAMPLE_P - 60, "-", "geneB"),
                      (SAMPLE_P + 1, 40, 0, SAMPLE_P + 1, "+", "."), (SAMPLE_P + 1500 - 30, 20, 0, SAMPLE_P + 1500 - 30, "-", "geneD")]
        self.gene_counts = codons_ref.codon_count(self.g, self.rows, codons_ref.regions_of(self.genes))
        base = self.frames[0][1] + self.frames[1][1]                      # SAMPLE_P = 2 mod 3: the third frame
        assert SAMPLE_P % 3 == 2
        first, second = self.counts[base + (SAMPLE_P - 2) // 3], self.counts[base + (SAMPLE_P + 63 - 2) // 3]
        self.double, self.triple = int(first[alt_triplet(self.g, SAMPLE_P, (0, 2))]), int(second[alt_triplet(self.g, SAMPLE_P + 63, (0, 1, 2))])
        assert self.tallies["placed"] > 1500, self.tallies
        assert sum(1 for r in self.rows if len(r[3]) == 8) >= 1, "no record with exactly 8 mismatches"
        assert int(first.sum()) > 100 and self.double > 50, (first.sum(), self.double)          # (161 and 108 as this was written)
        assert int(second.sum()) > 100 and self.triple > 50, (second.sum(), self.triple)        # (146 and 99)
