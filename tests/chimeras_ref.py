"""The chimera rule of `bronko call --chimeras`, restated in plain Python (include/bronko_hip.h bk_chimeras_enable, DESIGN.md
section X).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_chimera_events) and the
engine (chimera_scan_kernel) are held against it.  The genome, its anchor k-mers and a read's records are indels_ref's (the rule
takes them over word for word); everything from the two end anchors on is stated here.
"""
from __future__ import annotations

from dataclasses import dataclass

from tests.indels_ref import Genome, read_fasta, records_of, revcomp  # noqa: F401  (re-exported for the tests)

_ACGT = set("ACGT")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
L, R = 0, 1
SIDE_NAME = "LR"
TALLIES = ("records", "same_strand", "ref_spanning", "crossed", "supporting", "discordant")


@dataclass
class Result:
    events: dict        # (lo, side_lo, hi, side_hi) -> [lo_first, hi_first]
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


def _one_sequence(g: Genome, rec: str, front, back, M: int, res: Result) -> None:
    """Both anchors in one sequence: what the span needs of a record on one strand, nothing of any other."""
    k, n = g.k, len(rec)
    if front[2] != back[2]:
        return
    if front[2]:   # r' = the record along the reference: the anchors swap ends
        r = revcomp(rec)
        a, ca = n - k - back[0], back[1]
        b, cb = n - k - front[0], front[1]
    else:
        r = rec
        a, ca = front[0], front[1]
        b, cb = back[0], back[1]
    if a + k > b:
        return
    res.counters["same_strand"] += 1
    dL, dR = ca - a, cb - b
    s = g.seq_of(ca)
    lo, hi = min(dL, dR), max(dL, dR) + n
    if lo < g.first[s] or hi > g.first[s] + len(g.seqs[s]):
        return
    if any(g.text[x] not in _ACGT for x in range(lo, hi)):
        return
    if dR != dL:
        return
    if sum(1 for j in range(n) if r[j] != g.text[dL + j]) > M:
        return
    res.counters["ref_spanning"] += 1
    res.span[dL + a + k] += 1
    res.span[dL + b + 1] -= 1


class Arm:
    """One arm of a crossed record: the cell of offset j is c0 + d * j, and the base the read shows of a cell."""

    def __init__(self, g: Genome, c0: int, d: int):
        self.g, self.c0, self.d = g, c0, d
        self.s = None

    def cell(self, j: int) -> int:
        return self.c0 + self.d * j

    def base(self, cell: int) -> str:
        c = self.g.text[cell]
        return c if self.d > 0 else _COMP[c]

    def holds(self, cell: int) -> bool:
        """the cell lies in the arm's sequence and holds ACGT"""
        g, s = self.g, self.s
        return g.first[s] <= cell < g.first[s] + len(g.seqs[s]) and g.text[cell] in _ACGT


def slide_run(arm_a: Arm, arm_b: Arm, x: int, y: int):
    """(t0, t1): the pairs (x + dA t, y + dB t), t0 <= t <= t1, are the ones the reference cannot tell from (x, y)."""
    da, db = arm_a.d, arm_b.d

    def up_allowed(t):   # from the pair of t to the pair of t + 1
        u, v = x + da * (t + 1), y + db * (t + 1)
        if not (arm_a.holds(u) and arm_b.holds(v)):
            return False
        return arm_a.base(u) == arm_b.base(y + db * t)

    t1 = 0
    while up_allowed(t1):
        t1 += 1
    t0 = 0
    while arm_a.holds(x + da * (t0 - 1)) and arm_b.holds(y + db * (t0 - 1)) and up_allowed(t0 - 1):
        t0 -= 1
    return t0, t1


def _event_of(arm_a: Arm, arm_b: Arm, x: int, y: int):
    """The normalised event (lo, side_lo, hi, side_hi) of the pair (x, y) and whether arm A lies at lo"""
    t0, t1 = slide_run(arm_a, arm_b, x, y)
    side_a = L if arm_a.d > 0 else R
    side_b = R if arm_b.d > 0 else L
    ends = [(x + arm_a.d * t, y + arm_b.d * t) for t in (t0, t1)]
    assert t0 == t1 or min(ends[0]) != min(ends[1])
    u, v = min(ends, key=min)
    if u < v:
        return (u, side_a, v, side_b), True
    return (v, side_b, u, side_a), False


def add_record(g: Genome, rec: str, M: int, res: Result) -> None:
    k, n = g.k, len(rec)
    c = res.counters
    c["records"] += 1
    if n < 2 * k:
        return
    front = _end_anchor(g, rec, [0, 8, 16, 24])
    back = _end_anchor(g, rec, [n - k, n - k - 8, n - k - 16, n - k - 24])
    if front is None or back is None:
        return
    (f, cf, sf), (gg, cg, sg) = front, back
    sx, sy = g.seq_of(cf), g.seq_of(cg)
    if sx == sy:
        _one_sequence(g, rec, front, back, M, res)
        return
    if f + k > gg:
        return
    c["crossed"] += 1
    arm_a = Arm(g, cf + k - 1 + f, -1) if sf else Arm(g, cf - f, 1)
    arm_b = Arm(g, cg + k - 1 + gg, -1) if sg else Arm(g, cg - gg, 1)
    arm_a.s, arm_b.s = sx, sy
    if not all(arm_a.holds(arm_a.cell(j)) for j in range(0, gg)):
        return
    if not all(arm_b.holds(arm_b.cell(j)) for j in range(f + k, n)):
        return
    best = None
    for p in range(f + k, gg + 1):
        m = sum(1 for j in range(0, p) if rec[j] != arm_a.base(arm_a.cell(j))) + sum(1 for j in range(p, n) if rec[j] != arm_b.base(arm_b.cell(j)))
        x, y = arm_a.cell(p - 1), arm_b.cell(p)
        key = (m, min(x, y))
        assert best is None or key != best[0]
        if best is None or key < best[0]:
            best = (key, x, y)
    (m, _), x, y = best
    if m > M:
        c["discordant"] += 1
        return
    c["supporting"] += 1
    key, a_at_lo = _event_of(arm_a, arm_b, x, y)
    e = res.events.setdefault(key, [0, 0])
    e[0 if a_at_lo else 1] += 1


def chimera_events(g: Genome, reads, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, M, res)
    return res


def _span_at(sums, cell: int, side: int) -> int:
    return sums[cell + 1] if side == L else sums[cell]


def table_rows(g: Genome, res: Result, min_reads: int = 1) -> list[tuple]:
    """The reported events as bk_chimera_record: (lo, hi, sides, lo_first, hi_first, span_lo, span_hi, 0), sorted."""
    sums = res.span_sums()
    out = []
    for (lo, s_lo, hi, s_hi), (lf, hf) in res.events.items():
        if lf + hf >= min_reads:
            out.append((lo, hi, s_lo | s_hi << 1, lf, hf, _span_at(sums, lo, s_lo), _span_at(sums, hi, s_hi), 0))
    return sorted(out)


def counters_tuple(res: Result) -> tuple:
    return tuple(res.counters[name] for name in TALLIES)


def _arms_of(g: Genome, lo: int, s_lo: int, hi: int, s_hi: int):
    """An event's two arms, the one at lo taken as arm A"""
    arm_a, arm_b = Arm(g, 0, 1 if s_lo == L else -1), Arm(g, 0, 1 if s_hi == R else -1)
    arm_a.s, arm_b.s = g.seq_of(lo), g.seq_of(hi)
    return arm_a, arm_b


def homology(g: Genome, lo: int, s_lo: int, hi: int, s_hi: int) -> int:
    """t1 - t0 of the event's run, from the reference alone"""
    t0, t1 = slide_run(*_arms_of(g, lo, s_lo, hi, s_hi), lo, hi)
    return t1 - t0


def freq_text(reads: int, span_lo: int, span_hi: int) -> str:
    t = 10000 * reads // (reads + max(span_lo, span_hi))
    return "%d.%04d" % (t // 10000, t % 10000)


def tsv_text(g: Genome, rows, M: int, min_reads: int, supporting: int, ref_spanning: int) -> str:
    """OUT/<stem>.chimeras.tsv of the rows (as table_rows gives them) and the sample's two tallies: ordered by (lo, side_lo, hi,
    side_hi)."""
    out = ["##chimera_max_mismatches=%d" % M, "##chimera_min_reads=%d" % min_reads, "##chimera_supporting=%d" % supporting,
           "##chimera_ref_spanning=%d" % ref_spanning,
           "chrom_lo\tpos_lo\tside_lo\tchrom_hi\tpos_hi\tside_hi\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology"]
    lines = []
    for (lo, hi, sides, lf, hf, sl, sh, _) in rows:
        s_lo, s_hi = sides & 1, sides >> 1
        x, y = g.seq_of(lo), g.seq_of(hi)
        lines.append(((lo, s_lo, hi, s_hi), [g.names[x], lo - g.first[x] + 1, SIDE_NAME[s_lo], g.names[y], hi - g.first[y] + 1, SIDE_NAME[s_hi], lf, hf, lf + hf,
                                             sl, sh, freq_text(lf + hf, sl, sh), homology(g, lo, s_lo, hi, s_hi)]))
    lines.sort(key=lambda v: v[0])
    out += ["\t".join(str(v) for v in x[1]) for x in lines]
    return "".join(line + "\n" for line in out)
