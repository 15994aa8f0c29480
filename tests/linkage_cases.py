"""Inputs of the linkage tests (tests/test_linkage_cpu.py, tests/test_gpu_linkage.py): crafted records on indel_cases' crafted
two-sequence genome with the sites that go with them, and a sample of reads of HPV16 drawn from two planted haplotypes.  What the
rule makes of them is linkage_ref's business."""
from __future__ import annotations

import os
import random

from tests import indel_cases, indels_ref, linkage_ref
from tests.indel_cases import mut_read

N_LEN = 150
START = 900            # most crafted records begin at this cell of the first sequence
HPV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "HPV16.fa")


def crafted_cases(k: int):
    """[(label, read)] on indel_cases.crafted_genome(k); every read is there along and against the reference (label + '/rc')."""
    (_, a), (_, b) = indel_cases.crafted_genome(k)
    n = N_LEN
    cases = [("plain", a[START:START + n]),
             ("ends", mut_read(a, START, n, subs=(0, n - 1))),                       # the anchors move to offset 8
             ("step_15_16", mut_read(a, START, n, subs=(15, 16))),                    # the sixteen-base steps' boundaries
             ("step_31_32", mut_read(a, START, n, subs=(31, 32))),
             ("step_47_64", mut_read(a, START, n, subs=(47, 48, 63, 64))),
             ("step_bounds", mut_read(a, START, n, subs=(15, 16, 31, 32))),           # (all four: no anchor offset is left at this end)
             ("n_160", mut_read(a, START, 160, subs=(159,))),
             ("n_157", mut_read(a, START, 157, subs=(144, 156))),
             ("n_2k", a[START:START + 2 * k]),
             ("n_2k_minus_1", a[START:START + 2 * k - 1]),
             ("apart_2", mut_read(a, START, n, subs=(70, 72))),                       # inside one k-mer
             ("apart_5", mut_read(a, START, n, subs=(70, 75))),
             ("deletion", mut_read(a, START - 70, n, dele=(START, 1))),               # not placed
             ("over_N", a[1250:1300] + "A" * 20 + a[1320:1400]),                      # (the index reads N as A: the anchors agree, the cells do not)
             ("split_at_N", a[1230:1400]),
             ("across_sequences", a[-75:] + b[:75]),
             ("on_duplicate", a[600:600 + n]),
             ("second_seq", mut_read(b, 100, n, subs=(10, 50))),
             ("second_seq_plain", b[100:100 + n]),
             ("end_of_first", mut_read(a, len(a) - n, n, subs=(n - 5,))),
             ("start_of_second", mut_read(b, 0, n, subs=(k + 5,)))]
    for m in (1, 2, 3, 8, 9):                          # exactly M and M + 1 mismatches for M = 0, 2, 8
        cases.append(("mm_%d" % m, mut_read(a, START, n, subs=tuple(40 + 9 * t for t in range(m)))))
    out = []
    for label, read in cases:
        out.append((label, read))
        out.append((label + "/rc", "".join(indels_ref._COMP.get(c, "N") for c in reversed(read))))
    return out


def crafted_sites(k: int):
    """Cells that go with crafted_cases: the first and the last cell of the records at START and one cell outside either end, the
    substituted cells, cells of the second sequence and either side of the border between the sequences."""
    (_, a), _ = indel_cases.crafted_genome(k)
    first_b = len(a)
    s = [START - 1, START, START + 15, START + 16, START + 31, START + 32, START + 40, START + 47, START + 48, START + 49, START + 63, START + 64, START + 70, START + 72, START + 75,
         START + N_LEN - 1, START + N_LEN, len(a) - 5, len(a) - 1, first_b, first_b + k + 5, first_b + 110, first_b + 150]
    return sorted(set(s))


HAP1 = (0, 3, 63, 203, 1500)       # offsets from SAMPLE_P: 3, 60 and 140 apart, one more beyond 1,000
HAP2 = (30, 100)
SAMPLE_P = 2000
SAMPLE_SPAN = (1700, 3800)
SAMPLE_SEED = 1


def sample_reads(g: str, seed: int = SAMPLE_SEED, n_reads: int = 2000, length: int = N_LEN):
    """(reads, cells of haplotype 1's substitutions, cells of haplotype 2's): reads of both strands from SAMPLE_SPAN of the genome,
    70 % from haplotype 1 and 30 % from haplotype 2, 0.5 % of the bases substituted."""
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
        start = rng.randrange(SAMPLE_SPAN[0], SAMPLE_SPAN[1] - length)
        out = list(haps[0 if rng.random() < 0.7 else 1][start:start + length])
        for o in range(length):
            if rng.random() < 0.005:
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
        r = "".join(out)
        reads.append(indels_ref.revcomp(r) if rng.random() < 0.5 else r)
    return reads, [SAMPLE_P + o for o in HAP1], [SAMPLE_P + o for o in HAP2]


class Planted:
    """HPV16 at k = 21, the planted sample and what the restatement makes of it (computed once, shared, left unchanged)."""

    def __init__(self, k: int = 21):
        self.k = k
        self.g = indels_ref.read_fasta(HPV, k)
        self.reads, self.hap1, self.hap2 = sample_reads(self.g.text)
        self.sites = sorted(self.hap1 + self.hap2)
        self.rows, self.tallies = linkage_ref.link_rows(self.g, self.reads, 8)
        self.pairs = linkage_ref.link_count(self.g, self.rows, self.sites, 1000)
        code = linkage_ref._CODE
        nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
        self.recs = [(c, self.g.text[c], nxt[self.g.text[c]]) for c in self.sites]   # the planted substitutions as VCF records
        both = coupled = repulsed = 0
        for a, b, c in self.pairs:
            ra, rb = code[self.g.text[a]], code[self.g.text[b]]
            aa, ab = code[nxt[self.g.text[a]]], code[nxt[self.g.text[b]]]
            if c[4 * aa + ab] > 0:
                coupled += 1
            if c[4 * aa + ab] == 0 and c[4 * ra + ab] > 0 and c[4 * aa + rb] > 0:
                repulsed += 1
            both += 1
        assert self.tallies["placed"] > 500, self.tallies
        assert coupled >= 3 and repulsed >= 1, (coupled, repulsed)
        assert any(len(r[3]) == 8 for r in self.rows), "no record with exactly 8 mismatches"
        assert self.tallies["discordant"] >= 0 and len(self.pairs) == both
