"""The copy-back rule of `bronko call --copybacks`, restated in plain Python (include/bronko_hip.h bk_copybacks_enable, DESIGN.md
section B).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_copyback_events) and the
engine (copyback_scan_kernel) are held against it.  The genome, its anchor k-mers and a read's records are indels_ref's (the rule
takes them over word for word); everything from the two end anchors on is stated here.
"""
from __future__ import annotations

from dataclasses import dataclass

from tests.indels_ref import Genome, read_fasta, records_of, revcomp  # noqa: F401  (re-exported for the tests)

_ACGT = set("ACGT")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
H, T = 0, 1
KIND_NAME = "HT"
TALLIES = ("records", "same_strand", "ref_spanning", "switched", "supporting", "discordant")


@dataclass
class Result:
    events: dict        # (kind, lo, hi) -> [lo_first, hi_first]
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


def _same_strand(g: Genome, rec: str, front, back, M: int, res: Result) -> None:
    """Both anchors on one strand: what the span needs, as the junction rule has it."""
    k, n = g.k, len(rec)
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
    if g.seq_of(cb) != s:
        return
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


def slide_run(g: Genome, kind: int, x: int, y: int):
    """(t0, t1): the pairs (x + t, y - t), t0 <= t <= t1, are the ones the reference cannot tell from (x, y)."""
    s = g.seq_of(x)
    lo_s, hi_s = g.first[s], g.first[s] + len(g.seqs[s])
    ref = g.text

    def cell_ok(c):
        return lo_s <= c < hi_s and ref[c] in _ACGT

    def up_allowed(u, v):   # from the pair (u, v) to (u + 1, v - 1)
        if not (cell_ok(u + 1) and cell_ok(v - 1)):
            return False
        return ref[u + 1] == _COMP[ref[v]] if kind == H else _COMP[ref[u]] == ref[v - 1]

    t1 = 0
    while up_allowed(x + t1, y - t1):
        t1 += 1
    t0 = 0
    while cell_ok(x + t0 - 1) and cell_ok(y - t0 + 1) and up_allowed(x + t0 - 1, y - t0 + 1):
        t0 -= 1
    return t0, t1


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
    if front[2] == back[2]:
        _same_strand(g, rec, front, back, M, res)
        return
    (f, cf, sf), (gg, cg, _) = front, back
    if f + k > gg:
        return
    c["switched"] += 1
    kind = T if sf else H
    ref = g.text
    if kind == H:
        def A(j): return cf - f + j
        def B(j): return cg + k - 1 + gg - j
        def base_a(j): return ref[A(j)]
        def base_b(j): return _COMP[ref[B(j)]]
    else:
        def A(j): return cf + k - 1 + f - j
        def B(j): return cg - gg + j
        def base_a(j): return _COMP[ref[A(j)]]
        def base_b(j): return ref[B(j)]
    s = g.seq_of(cf)
    if g.seq_of(cg) != s:
        return
    lo_s, hi_s = g.first[s], g.first[s] + len(g.seqs[s])
    for cell in [A(j) for j in range(0, gg)] + [B(j) for j in range(f + k, n)]:
        if cell < lo_s or cell >= hi_s or ref[cell] not in _ACGT:
            return
    best = None
    for p in range(f + k, gg + 1):
        m = sum(1 for j in range(0, p) if rec[j] != base_a(j)) + sum(1 for j in range(p, n) if rec[j] != base_b(j))
        x, y = A(p - 1), B(p)
        key = (m, min(x, y), p)
        if best is None or key < best[0]:
            best = (key, x, y)
    (m, _, _), x, y = best
    if m > M:
        c["discordant"] += 1
        return
    c["supporting"] += 1
    t0, t1 = slide_run(g, kind, x, y)
    first, second = (x + t0, y - t0), (x + t1, y - t1)
    if min(first) == min(second):
        assert sorted(first) == sorted(second), (first, second)
    pair = first if min(first) <= min(second) else second
    e = res.events.setdefault((kind, min(pair), max(pair)), [0, 0])
    e[0 if x <= y else 1] += 1


def copyback_events(g: Genome, reads, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, M, res)
    return res


def table_rows(g: Genome, res: Result, min_reads: int = 1, min_dist: int = 0) -> list[tuple]:
    """The reported events as bk_copyback_record: (lo, hi, kind, lo_first, hi_first, span_lo, span_hi, 0), sorted."""
    sums = res.span_sums()
    out = []
    for (kind, lo, hi), (lf, hf) in res.events.items():
        if lf + hf >= min_reads and hi - lo >= min_dist:
            off = 1 if kind == H else 0
            out.append((lo, hi, kind, lf, hf, sums[lo + off], sums[hi + off], 0))
    return sorted(out)


def counters_tuple(res: Result) -> tuple:
    return tuple(res.counters[name] for name in TALLIES)


def homology(g: Genome, kind: int, lo: int, hi: int) -> int:
    """t1 - t0 of the event's run, from the reference alone"""
    t0, t1 = slide_run(g, kind, lo, hi)
    return t1 - t0


def freq_text(reads: int, span_lo: int, span_hi: int) -> str:
    t = 10000 * reads // (reads + max(span_lo, span_hi))
    return "%d.%04d" % (t // 10000, t % 10000)


def tsv_text(g: Genome, rows, M: int, min_reads: int, min_dist: int) -> str:
    """OUT/<stem>.copybacks.tsv of the rows (as table_rows gives them): ordered by (sequence, kind, lo, hi)."""
    out = ["##copyback_max_mismatches=%d" % M, "##copyback_min_reads=%d" % min_reads, "##copyback_min_dist=%d" % min_dist,
           "chrom\tkind\tlo\thi\tdistance\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology"]
    lines = []
    for (lo, hi, kind, lf, hf, sl, sh, _) in rows:
        s = g.seq_of(lo)
        a, b = lo - g.first[s] + 1, hi - g.first[s] + 1
        lines.append((s, kind, lo, hi, [g.names[s], KIND_NAME[kind], a, b, hi - lo, lf, hf, lf + hf, sl, sh, freq_text(lf + hf, sl, sh), homology(g, kind, lo, hi)]))
    lines.sort(key=lambda v: v[:4])
    out += ["\t".join(str(v) for v in x[4]) for x in lines]
    return "".join(line + "\n" for line in out)
