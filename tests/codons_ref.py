"""The codon rule of `bronko call --codons`, restated in plain Python (include/bronko_hip.h bk_sample_codons).

Plain loops, written from the rule and not from the C++ or the kernels: the host twin (bh_codon_count, bh_codon_bed,
bh_write_codons_tsv) and the engine (codon_count_kernel, codon_finish_kernel) are held against it.  Rows are linkage_ref's:
(cell0, n, strand, ((offset, base), ...)).  A region is (cell0, n_codons), the forward-strand cells [cell0, cell0 + 3 n_codons);
the codons of all regions are numbered in the order the regions are given.  A gene is a region as a BED line gives it:
(cell0, n_codons, seq, start, strand, name).
"""
from __future__ import annotations

import gzip

import numpy as np

from tests.indels_ref import Genome
from tests.linkage_ref import base_at

MAX_REGIONS, MAX_CODONS = 4096, 1 << 18
LETTERS = "ACGT"
HEADER = ["chrom", "region", "strand", "codon", "pos", "ref_codon", "ref_aa", "alt_codon", "alt_aa", "count", "cover", "freq", "type"]

# the standard code (NCBI table 1), by amino acid
_BY_AA = {"F": "TTT TTC", "L": "TTA TTG CTT CTC CTA CTG", "I": "ATT ATC ATA", "M": "ATG", "V": "GTT GTC GTA GTG",
          "S": "TCT TCC TCA TCG AGT AGC", "P": "CCT CCC CCA CCG", "T": "ACT ACC ACA ACG", "A": "GCT GCC GCA GCG", "Y": "TAT TAC",
          "*": "TAA TAG TGA", "H": "CAT CAC", "Q": "CAA CAG", "N": "AAT AAC", "K": "AAA AAG", "D": "GAT GAC", "E": "GAA GAG",
          "C": "TGT TGC", "W": "TGG", "R": "CGT CGC CGA CGG AGA AGG", "G": "GGT GGC GGA GGG"}
CODE = {codon: aa for aa, codons in _BY_AA.items() for codon in codons.split()}
assert len(CODE) == 64
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def translate(triplet: str) -> str:
    return CODE[triplet]


def check_regions(g: Genome, regions) -> None:
    assert len(regions) <= MAX_REGIONS and sum(nc for _, nc in regions) <= MAX_CODONS
    for c0, nc in regions:
        assert nc >= 1 and 0 <= c0 and c0 + 3 * nc <= g.cells and g.seq_of(c0) == g.seq_of(c0 + 3 * nc - 1), (c0, nc)


def triplet_of(g: Genome, row, cell: int) -> int:
    """16 b0 + 4 b1 + b2 of a row that covers the cells cell, cell + 1, cell + 2."""
    return 16 * base_at(g, row, cell) + 4 * base_at(g, row, cell + 1) + base_at(g, row, cell + 2)


def codon_count(g: Genome, rows, regions) -> np.ndarray:
    """count[codon][triplet]: for each region, codon and row, if the row covers the codon's three cells, its triplet there.  (The
    loop over a region's codons leaves out those that lie wholly in front of the row or wholly behind it.)"""
    check_regions(g, regions)
    out = np.zeros((sum(nc for _, nc in regions), 64), np.uint32)
    base = 0
    for c0, nc in regions:
        for row in rows:
            lo, hi = row[0], row[0] + row[1]
            for i in range(max(0, (lo - c0) // 3 - 1), min(nc, (hi - c0) // 3 + 2)):
                c = c0 + 3 * i
                if lo <= c and c + 2 < hi:
                    out[base + i, triplet_of(g, row, c)] += 1
        base += nc
    return out


def codon_count_by_differences(g: Genome, rows, regions) -> np.ndarray:
    """The same table the way the kernels make it: per (row, region) +1 / -1 into a difference array over the codons, the triplets of
    the codons that hold a mismatch, and the reference's triplet as the prefix sum's cover less the codon's other counters."""
    check_regions(g, regions)
    n = sum(nc for _, nc in regions)
    out = np.zeros((n, 64), np.int64)
    diff = [0] * (n + 1)
    base = 0
    for c0, nc in regions:
        for row in rows:
            lo, hi = row[0], row[0] + row[1]
            f = 0 if lo <= c0 else -((c0 - lo) // 3)
            l = min(nc, (hi - c0) // 3) if hi > c0 else 0
            if f >= l:
                continue
            diff[base + f] += 1
            diff[base + l] -= 1
            for i in sorted({(lo + off - c0) // 3 for off, _ in row[3] if lo + off >= c0}):
                if f <= i < l:
                    out[base + i, triplet_of(g, row, c0 + 3 * i)] += 1
        base += nc
    cover, at, base = 0, 0, 0
    for c0, nc in regions:
        for i in range(nc):
            cover += diff[at]
            ref = g.text[c0 + 3 * i:c0 + 3 * i + 3]
            if all(x in LETTERS for x in ref):
                t = 16 * LETTERS.index(ref[0]) + 4 * LETTERS.index(ref[1]) + LETTERS.index(ref[2])
                assert out[at, t] == 0
                out[at, t] = cover - out[at].sum()
            else:
                assert cover == 0
            at += 1
    assert cover + diff[n] == 0
    return out.astype(np.uint32)


def read_bed(g: Genome, path: str):
    """The genes of a --codons BED file (plain or gzip): chrom, 0-based start, end, optional name, score, optional strand.  ValueError
    with the file and the line named for what the rule refuses."""
    opener = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    genes, codons = [], 0
    with opener(path, "rt") as fh:
        for no, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line or line.startswith("#") or line.startswith("track") or line.startswith("browser"):
                continue
            where = "%s: line %d" % (path, no)
            col = line.split("\t")
            if len(col) < 3 or not col[1].isdigit() or not col[2].isdigit():
                raise ValueError(where + ": not a BED line")
            start, end = int(col[1]), int(col[2])
            strand = col[5] if len(col) > 5 and col[5] not in ("", ".") else "+"
            if strand not in "+-" or end <= start or (end - start) % 3:
                raise ValueError(where + ": no coding region")
            if col[0] not in g.names:
                raise ValueError(where + ": chrom")
            for s, name in enumerate(g.names):
                if name == col[0]:
                    if end > len(g.seqs[s]):
                        raise ValueError(where + ": beyond the sequence")
                    genes.append((g.first[s] + start, (end - start) // 3, s, start, strand, col[3] if len(col) > 3 and col[3] else "."))
                    codons += (end - start) // 3
            if len(genes) > MAX_REGIONS or codons > MAX_CODONS:
                raise ValueError("%s: too many regions or codons" % path)
    return genes


def regions_of(genes):
    return [(g[0], g[1]) for g in genes]


def _as_read(fwd: str, strand: str) -> str:
    return "".join(_COMP[c] for c in reversed(fwd)) if strand == "-" else fwd


def tsv_text(g: Genome, genes, counts, M: int = 8, N: int = 5, F: float = 0.03) -> str:
    """OUT/<stem>.codons.tsv for the genes (read_bed) and the counters of regions_of(genes)."""
    out = ["##codon_max_mismatches=%d" % M, "##codon_min_reads=%d" % N, "##codon_min_freq=%g" % F, "\t".join(HEADER)]
    base = 0
    for c0, nc, seq, start, strand, name in genes:
        for j in range(1, nc + 1):                     # in the direction of translation
            d = nc - j if strand == "-" else j - 1     # the codon among the region's forward-strand codons
            row = [int(v) for v in counts[base + d]]
            cover = sum(row)
            ref = g.text[c0 + 3 * d:c0 + 3 * d + 3]
            for t in range(64):
                fwd = LETTERS[t >> 4] + LETTERS[(t >> 2) & 3] + LETTERS[t & 3]
                if fwd == ref or row[t] < N or not row[t] >= F * cover:
                    continue
                rc, ac = _as_read(ref, strand), _as_read(fwd, strand)
                ra, aa = translate(rc), translate(ac)
                kind = "synonymous" if aa == ra else "nonsense" if aa == "*" else "stop_lost" if ra == "*" else "missense"
                q = 10000 * row[t] // cover
                out.append("\t".join([g.names[seq], name, strand, str(j), str(start + 3 * d + 1), rc, ra, ac, aa, str(row[t]), str(cover),
                                      "%d.%04d" % (q // 10000, q % 10000), kind]))
        base += nc
    return "".join(line + "\n" for line in out)
