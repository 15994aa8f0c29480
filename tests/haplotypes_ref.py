"""The haplotype rule of `bronko call --haplotypes`, restated in plain Python (include/bronko_hip.h bk_sample_haplotypes, DESIGN.md
section H).

Plain loops, written from the rule and not from the C++ or the kernels: the host twin (bh_hap_count, bh_hap_regions,
bh_write_haplotypes_tsv) and the engine (hap_count_kernel, hap_finish_kernel) are held against it.  Rows are linkage_ref's:
(cell0, n, strand, ((offset, base), ...)).  A region is (cell0, len), the forward-strand cells [cell0, cell0 + len).  A haplotype is
a tuple of (offset from the region's first cell, base), ascending; () is the reference's.  A window is a region as the output names
it: (cell0, len, seq, start, name).
"""
from __future__ import annotations

import gzip

from tests.indels_ref import Genome

MAX_REGIONS, MAX_LEN = 4096, 65520
LETTERS = "ACGT"
HEADER = ["chrom", "start", "end", "name", "cover", "haplotypes", "rank", "count", "freq", "n_sub", "substitutions"]


def check_regions(g: Genome, regions) -> None:
    assert len(regions) <= MAX_REGIONS
    for c0, ln in regions:
        assert 1 <= ln <= MAX_LEN and 0 <= c0 and c0 + ln <= g.cells and g.seq_of(c0) == g.seq_of(c0 + ln - 1), (c0, ln)


def haplotype(row, c0: int, ln: int):
    """The row's haplotype in the region, or None if the row does not span it."""
    cell0, n, _, mm = row
    if not (cell0 <= c0 and c0 + ln <= cell0 + n):
        return None
    return tuple((cell0 + off - c0, b) for off, b in mm if c0 <= cell0 + off < c0 + ln)


def hap_count(g: Genome, rows, regions):
    """(cover, ref_count, entries): two lists in the regions' order and [(region, count, haplotype)] over the distinct non-empty
    haplotypes, by region, then by haplotype -- tuples compare as the rule orders lists, a proper prefix first."""
    check_regions(g, regions)
    cover, ref, entries = [0] * len(regions), [0] * len(regions), []
    for i, (c0, ln) in enumerate(regions):
        seen = {}
        for row in rows:
            h = haplotype(row, c0, ln)
            if h is None:
                continue
            cover[i] += 1
            if h:
                seen[h] = seen.get(h, 0) + 1
            else:
                ref[i] += 1
        entries.extend((i, seen[h], h) for h in sorted(seen))
    return cover, ref, entries


def windows(g: Genome, window: int, step: int = 0):
    """The --hap-window tiling: the windows [i step, i step + window) that lie wholly inside a sequence, over every sequence."""
    step = step or window
    assert 1 <= window <= MAX_LEN and step >= 1
    out = []
    for s, seq in enumerate(g.seqs):
        out.extend((g.first[s] + at, window, s, at, ".") for at in range(0, len(seq) - window + 1, step))
    assert len(out) <= MAX_REGIONS
    return out


def read_bed(g: Genome, path: str):
    """The windows of a --haplotypes BED file (plain or gzip): chrom, 0-based start, end, optional name; further columns are not looked
    at.  ValueError with the file and the line named for what the rule refuses."""
    opener = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    out = []
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
            if end <= start or end - start > MAX_LEN:
                raise ValueError(where + ": no region")
            if col[0] not in g.names:
                raise ValueError(where + ": chrom")
            for s, name in enumerate(g.names):
                if name == col[0]:
                    if end > len(g.seqs[s]):
                        raise ValueError(where + ": beyond the sequence")
                    out.append((g.first[s] + start, end - start, s, start, col[3] if len(col) > 3 and col[3] else "."))
            if len(out) > MAX_REGIONS:
                raise ValueError("%s: too many regions" % path)
    return out


def regions_of(wins):
    return [(w[0], w[1]) for w in wins]


def ranked(cover_i: int, ref_i: int, haps):
    """[(count, haplotype)] of one region, the reference's included: by count descending, then by haplotype ascending."""
    every = list(haps) + ([(ref_i, ())] if ref_i else [])
    assert sum(c for c, _ in every) == cover_i
    return sorted(every, key=lambda ch: (-ch[0], ch[1]))


def tsv_text(g: Genome, wins, cover, ref, entries, M: int = 8, N: int = 5, F: float = 0.03) -> str:
    """OUT/<stem>.haplotypes.tsv for the windows (read_bed, windows) and the table of regions_of(wins)."""
    out = ["##hap_max_mismatches=%d" % M, "##hap_min_reads=%d" % N, "##hap_min_freq=%g" % F, "\t".join(HEADER)]
    for i, (c0, ln, seq, start, name) in enumerate(wins):
        every = ranked(cover[i], ref[i], [(c, h) for r, c, h in entries if r == i])
        for rank, (count, h) in enumerate(every, 1):
            if count < N or not count >= F * cover[i]:
                continue
            q = 10000 * count // cover[i]
            subs = ",".join("%d%s>%s" % (start + off + 1, g.text[c0 + off], LETTERS[b]) for off, b in h) or "."
            out.append("\t".join([g.names[seq], str(start), str(start + ln), name, str(cover[i]), str(len(every)), str(rank), str(count),
                                  "%d.%04d" % (q // 10000, q % 10000), str(len(h)), subs]))
    return "".join(line + "\n" for line in out)


def stats(cover, ref, entries, text: str):
    """(lines written, regions without cover, distinct haplotypes) as the writer reports them"""
    return text.count("\n") - 4, sum(1 for c in cover if c == 0), len(entries) + sum(1 for r in ref if r)
