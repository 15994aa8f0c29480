"""The duplication rule of `bronko call --duplications`, restated in plain Python (include/bronko_hip.h bk_duplications_enable,
DESIGN.md section V).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_duplication_events) and the
engine (duplication_scan_kernel) are held against it.  The genome, its anchor k-mers and a read's records are indels_ref's (the
rule takes them over word for word); everything from the anchors on is stated here.
"""
from __future__ import annotations

from dataclasses import dataclass

from tests.indels_ref import Genome, read_fasta, records_of, revcomp  # noqa: F401  (re-exported for the tests)

_ACGT = set("ACGT")
TALLIES = ("records", "anchored", "ref_spanning", "supporting", "short", "forward", "discordant")


@dataclass
class Result:
    events: dict        # (pos, E) -> [fwd, rev]
    span: list          # the per-cell difference array (cells + 2 entries), NOT prefix-summed
    counters: dict      # TALLIES

    def span_sums(self) -> list[int]:
        out, acc = [], 0
        for v in self.span:
            acc += v
            out.append(acc)
        return out


def new_result(g: Genome) -> Result:
    return Result({}, [0] * (g.cells + 2), {name: 0 for name in TALLIES})


def _end_anchor(g: Genome, rec: str, offsets):
    """The first anchor k-mer among the offsets tried: (offset, cell, against) or None."""
    for o in offsets:
        if o < 0 or o + g.k > len(rec):
            break
        hit = g.anchor(rec[o:o + g.k])
        if hit is not None:
            return o, hit[0], hit[1]
    return None


def _stretch_floor(g: Genome, lo: int, cell: int) -> int:
    """The first cell of the stretch of ACGT letters, of the sequence that begins at lo, that holds `cell`"""
    assert g.text[cell] in _ACGT
    while cell - 1 >= lo and g.text[cell - 1] in _ACGT:
        cell -= 1
    return cell


def add_record(g: Genome, rec: str, L: int, M: int, res: Result) -> None:
    k, n = g.k, len(rec)
    c = res.counters
    c["records"] += 1
    if n < 2 * k:
        return
    front = _end_anchor(g, rec, [0, 8, 16, 24])
    back = _end_anchor(g, rec, [n - k, n - k - 8, n - k - 16, n - k - 24])
    if front is None or back is None or front[2] != back[2]:
        return
    against = front[2]
    if against:   # r' = the record along the reference: the anchors swap ends
        r = revcomp(rec)
        a, ca = n - k - back[0], back[1]
        b, cb = n - k - front[0], front[1]
    else:
        r = rec
        a, ca = front[0], front[1]
        b, cb = back[0], back[1]
    if a + k > b:
        return
    c["anchored"] += 1
    dL, dR = ca - a, cb - b
    delta = dR - dL
    s = g.seq_of(ca)
    if g.seq_of(cb) != s:          # ignored without a tally, before anything is asked of delta
        return
    lo, hi = g.first[s], g.first[s] + len(g.seqs[s])
    ref = g.text

    def clean(x0, x1):
        return all(ref[x] in _ACGT for x in range(x0, x1))

    if delta == 0:
        if dL < lo or dL + n > hi or not clean(dL, dL + n):
            return
        m = sum(1 for j in range(n) if r[j] != ref[dL + j])
        if m > M:
            c["discordant"] += 1
            return
        c["ref_spanning"] += 1
        res.span[dL + a + k] += 1
        res.span[dL + b + 1] -= 1
        return
    if delta > 0:
        c["forward"] += 1
        return
    if -L < delta:
        c["short"] += 1
        return
    E = -delta
    if not (lo <= dL and dR + n <= hi):
        return
    p0, p1 = max(a + k, lo - dR), min(b, hi - dL)
    if p0 > p1:
        return
    if not clean(dL, dL + p1) or not clean(dR + p0, dR + n):
        return
    best = best_p = None
    for p in range(p0, p1 + 1):
        m = sum(1 for j in range(0, p) if r[j] != ref[dL + j]) + sum(1 for j in range(p, n) if r[j] != ref[dR + j])
        if best is None or m < best:
            best, best_p = m, p
    if best > M:
        c["discordant"] += 1
        return
    pos = dL + best_p
    FL, FR = _stretch_floor(g, lo, pos - 1), _stretch_floor(g, lo, pos - E)
    while pos - 1 > FL and pos - E - 1 >= FR and ref[pos - 1] == ref[pos - E - 1]:
        pos -= 1
    c["supporting"] += 1
    res.events.setdefault((pos, E), [0, 0])[1 if against else 0] += 1


def duplication_events(g: Genome, reads, L: int = 33, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, L, M, res)
    return res


def table_rows(g: Genome, res: Result, min_reads: int = 1) -> list[tuple]:
    """The events with fwd + rev >= min_reads as bk_duplication_record: (cell, len, fwd, rev, span_start, span_end), sorted."""
    sums = res.span_sums()
    return sorted((pos, E, fwd, rev, sums[pos - E], sums[pos]) for (pos, E), (fwd, rev) in res.events.items() if fwd + rev >= min_reads)


def counters_tuple(res: Result) -> tuple:
    return tuple(res.counters[name] for name in TALLIES)


def bounds(g: Genome, pos: int, E: int):
    """[lo, hi) of the sequence an event lies in: the one of its first duplicated cell (pos itself may be hi)"""
    s = g.seq_of(pos - E)
    return s, g.first[s], g.first[s] + len(g.seqs[s])


def homology(g: Genome, pos: int, E: int) -> int:
    """How far the left-normalised event could slide right: the consecutive h < E with pos + h < hi, both letters ACGT, and
    ref[pos + h] = ref[pos - E + h]."""
    _, _, hi = bounds(g, pos, E)
    h = 0
    while h < E and pos + h < hi and g.text[pos + h] in _ACGT and g.text[pos - E + h] in _ACGT and g.text[pos + h] == g.text[pos - E + h]:
        h += 1
    return h


def freq_text(reads: int, span_start: int, span_end: int) -> str:
    t = 10000 * reads // (reads + max(span_start, span_end))
    return "%d.%04d" % (t // 10000, t % 10000)


def tsv_text(g: Genome, rows, L: int, M: int, min_reads: int) -> str:
    """OUT/<stem>.duplications.tsv of the rows (as table_rows gives them): ordered by (sequence, start, end)."""
    out = ["##duplication_min_len=%d" % L, "##duplication_max_mismatches=%d" % M, "##duplication_min_reads=%d" % min_reads,
           "chrom\tstart\tend\tlength\tfwd\trev\treads\tspan_start\tspan_end\tfreq\thomology\twhole"]
    lines = []
    for (pos, E, fwd, rev, ss, se) in rows:
        s, lo, hi = bounds(g, pos, E)
        start, end = pos - E - lo + 1, pos - lo
        lines.append((s, start, end, [g.names[s], start, end, E, fwd, rev, fwd + rev, ss, se, freq_text(fwd + rev, ss, se), homology(g, pos, E),
                                      1 if E == hi - lo else 0]))
    lines.sort(key=lambda x: x[:3])
    out += ["\t".join(str(v) for v in x[3]) for x in lines]
    return "".join(line + "\n" for line in out)
