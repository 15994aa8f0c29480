"""The breakend rule of `bronko call --breakends`, restated in plain Python (include/bronko_hip.h bk_breakends_enable, DESIGN.md
section E).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_breakend_events) and the
engine (breakend_scan_kernel) are held against it.  The genome, its anchor k-mers and a read's records are indels_ref's (the rule
takes them over word for word); everything from the end anchors on is stated here.
"""
from __future__ import annotations

from dataclasses import dataclass

from tests.indels_ref import Genome, read_fasta, records_of, revcomp, seq_code  # noqa: F401  (re-exported for the tests)

_ACGT = set("ACGT")
L, R = 0, 1
SIDE_NAME = "LR"
PENALTY = 4             # BK_BREAKEND_MISMATCH_PENALTY
TAG = 16
TALLIES = ("records", "one_anchor", "ref_spanning", "supporting", "short", "through", "discordant", "unplaced")


@dataclass
class Result:
    events: dict        # (cell, side, tag letters) -> [fwd, rev]
    span: list          # the per-cell difference array (cells + 2 entries), NOT prefix-summed
    counters: dict      # TALLIES

    def span_sums(self) -> list[int]:
        out, acc = [], 0
        for v in self.span:
            acc += v
            out.append(acc)
        return out

    def site_reads(self) -> dict:
        out = {}
        for (cell, side, _), (f, r) in self.events.items():
            out[(cell, side)] = out.get((cell, side), 0) + f + r
        return out


def new_result(g: Genome) -> Result:
    return Result({}, [0] * (g.cells + 2), {name: 0 for name in TALLIES})


def end_anchor(g: Genome, rec: str, offsets):
    """The first anchor k-mer among the offsets tried: (offset, cell, against) or None."""
    for o in offsets:
        if o < 0 or o + g.k > len(rec):
            break
        hit = g.anchor(rec[o:o + g.k])
        if hit is not None:
            return o, hit[0], hit[1]
    return None


def end_anchors(g: Genome, rec: str):
    n, k = len(rec), g.k
    return end_anchor(g, rec, [0, 8, 16, 24]), end_anchor(g, rec, [n - k, n - k - 8, n - k - 16, n - k - 24])


def _two_anchors(g: Genome, rec: str, front, back, M: int, res: Result) -> None:
    """Both ends anchored: what the span needs, nothing else."""
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
    s = g.seq_of(ca)
    if g.seq_of(cb) != s:
        return
    dL, dR = ca - a, cb - b
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


def stretch(g: Genome, c: int):
    """[lo, hi): the cells around c that belong to c's sequence and hold ACGT, without a gap; empty where c holds another letter"""
    s = g.seq_of(c)
    first, end = g.first[s], g.first[s] + len(g.seqs[s])
    if g.text[c] not in _ACGT:
        return c, c
    lo = c
    while lo - 1 >= first and g.text[lo - 1] in _ACGT:
        lo -= 1
    hi = c + 1
    while hi < end and g.text[hi] in _ACGT:
        hi += 1
    return lo, hi


def classify(g: Genome, rec: str, C: int, M: int):
    """A record of one anchor: ('unplaced' | 'discordant' | 'through' | 'short', None) or ('supporting', (cell, side, tag, against))"""
    k, n = g.k, len(rec)
    front, back = end_anchors(g, rec)
    assert (front is None) != (back is None)
    off, c, against = front if front is not None else back
    r = revcomp(rec) if against else rec
    a = n - k - off if against else off
    d = c - a
    side = L if (front is not None) != against else R
    lo, hi = stretch(g, c)
    if not (lo <= c and c + k <= hi):
        return "unplaced", None
    if side == L:
        if d < lo:
            return "unplaced", None
        P = min(n, hi - d)
        scores = {p: (p - a - k) - (PENALTY + 1) * sum(1 for j in range(a + k, p) if r[j] != g.text[d + j]) for p in range(a + k, P + 1)}
        top = max(scores.values())
        edge = min(p for p, v in scores.items() if v == top)
        held = range(0, edge)
        clip = n - edge
    else:
        if d + n > hi:
            return "unplaced", None
        Q = max(0, lo - d)
        scores = {q: (a - q) - (PENALTY + 1) * sum(1 for j in range(q, a) if r[j] != g.text[d + j]) for q in range(Q, a + 1)}
        top = max(scores.values())
        edge = max(q for q, v in scores.items() if v == top)
        held = range(edge, n)
        clip = edge
    assert all(lo <= d + j < hi for j in held)
    if sum(1 for j in held if r[j] != g.text[d + j]) > M:
        return "discordant", None
    if clip == 0:
        return "through", None
    if clip < C:
        return "short", None
    if side == L:
        return "supporting", (d + edge - 1, L, r[edge:edge + TAG], against)
    return "supporting", (d + edge, R, r[edge - TAG:edge], against)


def add_record(g: Genome, rec: str, C: int, M: int, res: Result) -> None:
    k, n = g.k, len(rec)
    c = res.counters
    c["records"] += 1
    if n < 2 * k:
        return
    front, back = end_anchors(g, rec)
    if front is None and back is None:
        return
    if front is not None and back is not None:
        _two_anchors(g, rec, front, back, M, res)
        return
    c["one_anchor"] += 1
    what, ev = classify(g, rec, C, M)
    c[what] += 1
    if ev is not None:
        cell, side, tag, against = ev
        assert len(tag) == TAG
        e = res.events.setdefault((cell, side, tag), [0, 0])
        e[1 if against else 0] += 1


def breakend_events(g: Genome, reads, C: int = 20, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    assert 16 <= C <= 65519 and 0 <= M <= 8
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, C, M, res)
    return res


def _span_at(sums, cell: int, side: int) -> int:
    return sums[cell + 1] if side == L else sums[cell]


def table_rows(g: Genome, res: Result, min_reads: int = 1) -> list[tuple]:
    """The reported events as bk_breakend_record: (cell, tag, side, fwd, rev, site_reads, span, 0), sorted."""
    sums, site = res.span_sums(), res.site_reads()
    out = []
    for (cell, side, tag), (f, r) in res.events.items():
        if f + r >= min_reads:
            out.append((cell, seq_code(tag), side, f, r, site[(cell, side)], _span_at(sums, cell, side), 0))
    return sorted(out)


def counters_tuple(res: Result) -> tuple:
    return tuple(res.counters[name] for name in TALLIES)


def tallies10(res: Result, min_reads: int) -> tuple:
    """What the ##breakend_tallies line prints: the eight tallies, the distinct events, the reported ones"""
    return counters_tuple(res) + (len(res.events), sum(1 for f, r in res.events.values() if f + r >= min_reads))


def tag_letters(tag: int) -> str:
    return "".join("ACGT"[(tag >> (2 * t)) & 3] for t in range(TAG))


def freq_text(reads: int, span: int) -> str:
    t = 10000 * reads // (reads + span)
    return "%d.%04d" % (t // 10000, t % 10000)


def tsv_text(g: Genome, rows, C: int, M: int, min_reads: int, tallies) -> str:
    """OUT/<stem>.breakends.tsv of the rows (as table_rows gives them) and the sample's ten tallies: ordered by (cell, side, tag)."""
    names = TALLIES + ("candidates", "reported")
    out = ["##breakend_min_clip=%d" % C, "##breakend_max_mismatches=%d" % M, "##breakend_min_reads=%d" % min_reads,
           "##breakend_tallies=" + ",".join("%s:%d" % (n, v) for n, v in zip(names, tallies)),
           "chrom\tpos\tside\tfwd\trev\treads\tsite_reads\tspan\tfreq\tterminus\ttag"]
    lines = []
    for (cell, tag, side, f, r, site, span, _) in rows:
        s = g.seq_of(cell)
        last = g.first[s] + len(g.seqs[s]) - 1
        terminus = 1 if (side == R and cell == g.first[s]) or (side == L and cell == last) else 0
        letters = tag_letters(tag)
        lines.append(((cell, side, letters), [g.names[s], cell - g.first[s] + 1, SIDE_NAME[side], f, r, f + r, site, span, freq_text(f + r, span), terminus, letters]))
    lines.sort(key=lambda v: v[0])
    out += ["\t".join(str(v) for v in x[1]) for x in lines]
    return "".join(line + "\n" for line in out)
