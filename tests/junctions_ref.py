"""The junction rule of `bronko call --junctions`, restated in plain Python (include/bronko_hip.h bk_junctions_enable, DESIGN.md
section J).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_junction_events) and the
engine (junction_scan_kernel) are held against it.  The genome, its anchor k-mers and a read's records are indels_ref's (the rule
takes them over word for word); everything from the anchors on is stated here.
"""
from __future__ import annotations

from dataclasses import dataclass

from tests.indels_ref import Genome, read_fasta, records_of, revcomp  # noqa: F401  (re-exported for the tests)

_ACGT = set("ACGT")
TALLIES = ("records", "anchored", "ref_spanning", "supporting", "short", "backward", "discordant")


@dataclass
class Result:
    events: dict        # (pos, D) -> [fwd, rev]
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
    # ignored without a tally
    s = g.seq_of(ca)
    if g.seq_of(cb) != s:
        return
    lo, hi = min(dL, dR), max(dL, dR) + n
    if lo < g.first[s] or hi > g.first[s] + len(g.seqs[s]):
        return
    ref = g.text
    if any(ref[x] not in _ACGT for x in range(lo, hi)):
        return
    if delta == 0:
        m = sum(1 for j in range(n) if r[j] != ref[dL + j])
        if m > M:
            c["discordant"] += 1
            return
        c["ref_spanning"] += 1
        res.span[dL + a + k] += 1
        res.span[dL + b + 1] -= 1
        return
    if abs(delta) < L:
        c["short"] += 1
        return
    if delta <= -L:
        c["backward"] += 1
        return
    D = delta
    best = best_p = None
    for p in range(a + k, b + 1):
        m = sum(1 for j in range(0, p) if r[j] != ref[dL + j]) + sum(1 for j in range(p, n) if r[j] != ref[dR + j])
        if best is None or m < best:
            best, best_p = m, p
    if best > M:
        c["discordant"] += 1
        return
    pos = dL + best_p
    F = pos - 1   # the first cell of the stretch of ACGT letters of this sequence that holds pos - 1
    while F - 1 >= g.first[s] and ref[F - 1] in _ACGT:
        F -= 1
    while pos - 1 > F and ref[pos - 1] == ref[pos + D - 1]:
        pos -= 1
    c["supporting"] += 1
    res.events.setdefault((pos, D), [0, 0])[1 if against else 0] += 1


def junction_events(g: Genome, reads, L: int = 33, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, L, M, res)
    return res


def table_rows(g: Genome, res: Result, min_reads: int = 1) -> list[tuple]:
    """The events with fwd + rev >= min_reads as bk_junction_record: (cell, len, fwd, rev, span_donor, span_acceptor), sorted."""
    sums = res.span_sums()
    return sorted((pos, D, fwd, rev, sums[pos], sums[pos + D]) for (pos, D), (fwd, rev) in res.events.items() if fwd + rev >= min_reads)


def counters_tuple(res: Result) -> tuple:
    return tuple(res.counters[name] for name in TALLIES)


def homology(g: Genome, pos: int, D: int) -> int:
    """How far the left-normalised junction could slide right: the consecutive j < D with ref[pos + j] = ref[pos + D + j], inside the
    sequence, both letters ACGT."""
    s = g.seq_of(pos)
    end = g.first[s] + len(g.seqs[s])
    h = 0
    while h < D and pos + D + h < end and g.text[pos + h] in _ACGT and g.text[pos + h] == g.text[pos + D + h]:
        h += 1
    return h


def freq_text(reads: int, span_donor: int) -> str:
    t = 10000 * reads // (reads + span_donor)
    return "%d.%04d" % (t // 10000, t % 10000)


def tsv_text(g: Genome, rows, L: int, M: int, min_reads: int) -> str:
    """OUT/<stem>.junctions.tsv of the rows (as table_rows gives them): ordered by (sequence, donor, acceptor)."""
    out = ["##junction_min_len=%d" % L, "##junction_max_mismatches=%d" % M, "##junction_min_reads=%d" % min_reads,
           "chrom\tdonor\tacceptor\tlength\tfwd\trev\treads\tspan_donor\tspan_acceptor\tfreq\thomology"]
    lines = []
    for (pos, D, fwd, rev, sd, sa) in rows:
        s = g.seq_of(pos)
        donor = pos - g.first[s]
        lines.append((s, donor, donor + D + 1, [g.names[s], donor, donor + D + 1, D, fwd, rev, fwd + rev, sd, sa, freq_text(fwd + rev, sd), homology(g, pos, D)]))
    lines.sort(key=lambda x: x[:3])
    out += ["\t".join(str(v) for v in x[3]) for x in lines]
    return "".join(line + "\n" for line in out)
