"""The linkage rule of `bronko call --linkage`, restated in plain Python (include/bronko_hip.h).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_link_rows, bh_link_count)
and the engine (link_scan_kernel, link_count_kernel) are held against it.  Cells are the positions of all sequences of the genome
file, concatenated.  A row is (cell0, n, strand, ((offset, base), ...)) with the mismatches ascending by offset.
"""
from __future__ import annotations

from tests.indels_ref import Genome, records_of, revcomp

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
MAX_SITES, MAX_PAIRS = 65536, 1 << 20


def place(g: Genome, rec: str, M: int):
    """('placed', row), ('unplaced', None) or ('discordant', None) of one record."""
    k, n = g.k, len(rec)
    if n < 2 * k:
        return "unplaced", None
    front = back = None
    for t in range(4):
        o = 8 * t
        if o + k > n:
            break
        hit = g.anchor(rec[o:o + k])
        if hit is not None:
            front = (o, hit)
            break
    for t in range(4):
        o = n - k - 8 * t
        if o < 0:
            break
        hit = g.anchor(rec[o:o + k])
        if hit is not None:
            back = (o, hit)
            break
    if front is None or back is None or front[1][1] != back[1][1]:
        return "unplaced", None
    against = front[1][1]
    if against:   # r' = the record along the reference
        r = revcomp(rec)
        a, ca = n - k - back[0], back[1][0]
        b, cb = n - k - front[0], front[1][0]
    else:
        r = rec
        a, ca = front[0], front[1][0]
        b, cb = back[0], back[1][0]
    if a + k > b:
        return "unplaced", None
    dL, dR = ca - a, cb - b
    if dR != dL:
        return "unplaced", None
    s = g.seq_of(ca)
    if g.seq_of(cb) != s:
        return "unplaced", None
    if dL < g.first[s] or dL + n > g.first[s] + len(g.seqs[s]):
        return "unplaced", None
    if any(g.text[c] not in _CODE for c in range(dL, dL + n)):
        return "unplaced", None
    mm = tuple((j, _CODE[r[j]]) for j in range(n) if r[j] != g.text[dL + j])
    if len(mm) > M:
        return "discordant", None
    return "placed", (dL, n, 1 if against else 0, mm)


def link_rows(g: Genome, reads, M: int = 8):
    """(rows sorted, tallies) of every record of every read (strings; split here at non-ACGT letters)."""
    rows, t = [], dict(records=0, placed=0, unplaced=0, discordant=0)
    for read in reads:
        for rec in records_of(read, g.k):
            t["records"] += 1
            what, row = place(g, rec, M)
            t[what] += 1
            if row is not None:
                rows.append(row)
    rows.sort()
    return rows, t


def pairs_of(g: Genome, sites, max_dist: int):
    """[(i, j)] in (i, j) order: i < j, both cells in one sequence, at most max_dist apart."""
    assert all(x < y for x, y in zip(sites, sites[1:])) and len(sites) <= MAX_SITES
    out = []
    for i in range(len(sites)):
        for j in range(i + 1, len(sites)):
            if sites[j] - sites[i] > max_dist:
                break
            if g.seq_of(sites[i]) == g.seq_of(sites[j]):
                out.append((i, j))
    assert len(out) <= MAX_PAIRS
    return out


def base_at(g: Genome, row, cell: int) -> int:
    cell0, n, _, mm = row
    assert cell0 <= cell < cell0 + n
    for off, b in mm:
        if off == cell - cell0:
            return b
    return _CODE[g.text[cell]]


def link_count(g: Genome, rows, sites, max_dist: int = 1000):
    """[(site_a, site_b, [16 counters])] in (i, j) order; counter 4 * bA + bB."""
    pairs = pairs_of(g, sites, max_dist)
    counts = {p: [0] * 16 for p in pairs}
    for row in rows:
        covered = [i for i, c in enumerate(sites) if row[0] <= c < row[0] + row[1]]
        for x, i in enumerate(covered):
            for j in covered[x + 1:]:
                if (i, j) in counts:
                    counts[(i, j)][4 * base_at(g, row, sites[i]) + base_at(g, row, sites[j])] += 1
    return [(sites[i], sites[j], counts[(i, j)]) for i, j in pairs]


def parse_vcf(g: Genome, text: str):
    """[(cell, ref letter, alt letter)] of the substitution records of a VCF's text."""
    out = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        s = g.names.index(f[0])
        out.append((g.first[s] + int(f[1]) - 1, f[3], f[4]))
    return out


def sites_of(recs):
    return sorted({r[0] for r in recs})


def tsv_text(g: Genome, recs, pairs, M: int = 8, D: int = 1000, N: int = 1) -> str:
    """OUT/<stem>.linkage.tsv for the VCF records `recs` (parse_vcf) and the counted `pairs` (link_count of sites_of(recs))."""
    out = ["##link_max_mismatches=%d" % M, "##link_max_dist=%d" % D, "##link_min_reads=%d" % N,
           "\t".join(["chrom", "pos_a", "ref_a", "alt_a", "pos_b", "ref_b", "alt_b", "cover", "ref_ref", "ref_alt", "alt_ref", "alt_alt", "other"])]
    counted = {(a, b): c for a, b, c in pairs}
    recs = sorted(recs, key=lambda r: (r[0], _CODE[r[2]]))
    for x, (ca, ra, aa) in enumerate(recs):
        for cb, rb, ab in recs[x + 1:]:
            c = counted.get((ca, cb))
            if cb == ca or c is None or sum(c) < N:
                continue
            s = g.seq_of(ca)
            four = [c[4 * _CODE[ra] + _CODE[rb]], c[4 * _CODE[ra] + _CODE[ab]], c[4 * _CODE[aa] + _CODE[rb]], c[4 * _CODE[aa] + _CODE[ab]]]
            out.append("\t".join([g.names[s], str(ca - g.first[s] + 1), ra, aa, str(cb - g.first[s] + 1), rb, ab, str(sum(c))] +
                                 [str(v) for v in four] + [str(sum(c) - sum(four))]))
    return "".join(line + "\n" for line in out)
