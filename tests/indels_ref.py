"""The indel rule of `bronko call --indels`, restated in plain Python (include/bronko_hip.h).

Plain loops over strings, written from the rule and not from the C++ or the kernels: the host twin (bh_indel_events) and the
engine (indel_scan_kernel) are held against it.  Cells are the positions of all sequences of the genome file, concatenated.
"""
from __future__ import annotations

from dataclasses import dataclass, field

DEL, INS = 0, 1
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def revcomp(s: str) -> str:
    return "".join(_COMP[c] for c in reversed(s))


def records_of(read: str, k: int) -> list[str]:
    """A read's records: its runs of ACGT letters of at least k bases."""
    out, run = [], []
    for c in read.upper() + "N":
        if c in _CODE:
            run.append(c)
        else:
            if len(run) >= k:
                out.append("".join(run))
            run = []
    return out


def seq_code(s: str) -> int:
    """An inserted sequence as the ABI's 64 bits: base t at bits [2t, 2t + 2), A C G T = 0 1 2 3."""
    v = 0
    for t, c in enumerate(s):
        v |= _CODE[c] << (2 * t)
    return v


@dataclass
class Genome:
    """One genome file: names and letters of its sequences, and what the rule derives from them."""
    names: list[str]
    seqs: list[str]                      # upper-cased letters as the FASTA has them
    k: int
    first: list[int] = field(default_factory=list)   # first cell of each sequence
    text: str = ""                       # all cells
    unique: dict = field(default_factory=dict)       # canonical k-mer -> (cell, reverse-complemented there), the anchor k-mers

    def __post_init__(self):
        self.seqs = [s.upper() for s in self.seqs]
        at = 0
        for s in self.seqs:
            self.first.append(at)
            at += len(s)
        self.text = "".join(self.seqs)
        # the genome's k-mers as the index reads them: every letter that is not ACGT stands for A
        seen: dict[str, list] = {}
        for f, s in zip(self.first, self.seqs):
            idx = "".join(c if c in _CODE else "A" for c in s)
            for i in range(len(s) - self.k + 1):
                kmer = idx[i:i + self.k]
                rc = revcomp(kmer)
                canon, is_rc = (kmer, False) if kmer < rc else (rc, True)
                e = seen.setdefault(canon, [0, f + i, is_rc])
                e[0] += 1
        self.unique = {c: (e[1], e[2]) for c, e in seen.items() if e[0] == 1}

    @property
    def cells(self) -> int:
        return len(self.text)

    def seq_of(self, cell: int) -> int:
        s = 0
        while s + 1 < len(self.first) and self.first[s + 1] <= cell:
            s += 1
        return s

    def anchor(self, kmer: str):
        """(cell, against the reference) of an anchor k-mer, or None."""
        rc = revcomp(kmer)
        canon, read_rc = (kmer, False) if kmer < rc else (rc, True)
        hit = self.unique.get(canon)
        if hit is None:
            return None
        return hit[0], read_rc != hit[1]


def read_fasta(path, k: int) -> Genome:
    names, seqs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                names.append(line[1:].split()[0] if line[1:].split() else "")
                seqs.append([])
            elif seqs:
                seqs[-1].append(line)
    return Genome(names, ["".join(s) for s in seqs], k)


@dataclass
class Result:
    events: dict        # (cell, kind, length, S) -> [fwd, rev]
    span: list          # the per-cell difference array (cells + 2 entries), NOT prefix-summed
    counters: dict      # records, anchored, ref_spanning, supporting, discordant

    def span_sums(self) -> list[int]:
        out, acc = [], 0
        for v in self.span:
            acc += v
            out.append(acc)
        return out


def new_result(g: Genome) -> Result:
    return Result({}, [0] * (g.cells + 2), dict(records=0, anchored=0, ref_spanning=0, supporting=0, discordant=0))


def add_record(g: Genome, rec: str, L: int, M: int, res: Result) -> None:
    k, n = g.k, len(rec)
    res.counters["records"] += 1
    if n < 2 * k:
        return
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
        return
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
        return
    res.counters["anchored"] += 1
    dL, dR = ca - a, cb - b
    delta = dR - dL
    if abs(delta) > L:
        res.counters["discordant"] += 1
        return
    s = g.seq_of(ca)
    if g.seq_of(cb) != s:
        return
    lo, hi = min(dL, dR), max(dL, dR) + n
    if lo < g.first[s] or hi > g.first[s] + len(g.seqs[s]):
        return
    ref = g.text
    if any(ref[c] not in _CODE for c in range(lo, hi)):
        return

    def floor_of(pos):   # first cell of the stretch of ACGT letters of this sequence that holds pos - 1
        f = pos - 1
        while f - 1 >= g.first[s] and ref[f - 1] in _CODE:
            f -= 1
        return f

    if delta == 0:
        m = sum(1 for j in range(n) if r[j] != ref[dL + j])
        if m > M:
            res.counters["discordant"] += 1
            return
        res.counters["ref_spanning"] += 1
        res.span[dL + a + k] += 1
        res.span[dL + b + 1] -= 1
        return
    if delta > 0:
        D = delta
        best, best_p = None, None
        for p in range(a + k, b + 1):
            m = sum(1 for j in range(p) if r[j] != ref[dL + j]) + sum(1 for j in range(p, n) if r[j] != ref[dR + j])
            if best is None or m < best:
                best, best_p = m, p
        if best > M:
            res.counters["discordant"] += 1
            return
        pos = dL + best_p
        F = floor_of(pos)
        while pos - 1 > F and ref[pos - 1] == ref[pos + D - 1]:
            pos -= 1
        key = (pos, DEL, D, "")
    else:
        I = -delta
        if a + k > b - I:
            res.counters["discordant"] += 1
            return
        best, best_p = None, None
        for p in range(a + k, b - I + 1):
            m = sum(1 for j in range(p) if r[j] != ref[dL + j]) + sum(1 for j in range(p + I, n) if r[j] != ref[dR + j])
            if best is None or m < best:
                best, best_p = m, p
        if best > M:
            res.counters["discordant"] += 1
            return
        S = r[best_p:best_p + I]
        pos = dL + best_p
        F = floor_of(pos)
        while pos - 1 > F and ref[pos - 1] == S[-1]:
            S = S[-1] + S[:-1]
            pos -= 1
        key = (pos, INS, I, S)
    res.counters["supporting"] += 1
    e = res.events.setdefault(key, [0, 0])
    e[1 if against else 0] += 1


def indel_events(g: Genome, reads, L: int = 32, M: int = 2, res: Result | None = None) -> Result:
    """Every record of every read (strings; split here at non-ACGT letters) into the sample's table and span array."""
    res = res if res is not None else new_result(g)
    for read in reads:
        for rec in records_of(read, g.k):
            add_record(g, rec, L, M, res)
    return res


def table_rows(g: Genome, res: Result) -> list[tuple]:
    """The whole table as the engine downloads it at min_reads 1, ppm 0: (cell, len, fwd, rev, ref_span, seq), sorted by
    (cell, kind, length, seq); len > 0 a deletion, < 0 an insertion."""
    sums = res.span_sums()
    rows = []
    for (cell, kind, length, S), (fwd, rev) in res.events.items():
        rows.append((cell, kind, length, seq_code(S), fwd, rev, sums[cell]))
    rows.sort(key=lambda r: r[:4])
    return [(c, ln if kd == DEL else -ln, f, rv, rs, sq) for (c, kd, ln, sq, f, rv, rs) in rows]


def report(g: Genome, res: Result, min_reads: int, min_af_ppm: int) -> list[tuple]:
    """The reported events: (cell, kind, length, S, fwd, rev, ref_span), sorted by (cell, kind, length, seq)."""
    sums = res.span_sums()
    out = []
    for (cell, kind, length, S), (fwd, rev) in res.events.items():
        support, rs = fwd + rev, sums[cell]
        if support >= min_reads and support * 1_000_000 >= min_af_ppm * (support + rs):
            out.append((cell, kind, length, S, fwd, rev, rs))
    out.sort(key=lambda r: (r[0], r[1], r[2], seq_code(r[3])))
    return out


def af_text(support: int, ref_span: int) -> str:
    t = 10000 * support // (support + ref_span)
    return "%d.%04d" % (t // 10000, t % 10000)


def vcf_header(g: Genome, reads_path: str, L: int, M: int, min_reads: int, min_af_ppm: int) -> list[str]:
    """The header of OUT/<stem>.indels.vcf: the main VCF's lines that apply, the INFO lines, the four parameters, the columns."""
    out = ["##fileformat=VCFv4.5", "##source=bronko-v0.1.0", "##reference=file://" + reads_path]
    out += ["##contig=<ID=%s,length=%d>" % (name, len(s)) for name, s in zip(g.names, g.seqs)]
    out += ['##INFO=<ID=TYPE,Number=1,Type=String,Description="DEL or INS">',
            '##INFO=<ID=LEN,Number=1,Type=Integer,Description="Bases deleted or inserted">',
            '##INFO=<ID=SF,Number=1,Type=Integer,Description="Supporting records along the reference">',
            '##INFO=<ID=SR,Number=1,Type=Integer,Description="Supporting records against the reference">',
            '##INFO=<ID=RS,Number=1,Type=Integer,Description="Records that span the site without an indel">',
            '##INFO=<ID=AF,Number=1,Type=Float,Description="(SF + SR) / (SF + SR + RS)">',
            "##indel_max_len=%d" % L, "##indel_max_mismatches=%d" % M, "##indel_min_reads=%d" % min_reads,
            "##indel_min_af=%d.%06d" % (min_af_ppm // 1000000, min_af_ppm % 1000000),
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    return out


def vcf_text(g: Genome, rows, header_lines: list[str], sample: str | None = None) -> str:
    """The body under the given header lines (the caller passes every `##` line and the column line)."""
    out = list(header_lines)
    for (cell, kind, length, S, fwd, rev, rs) in rows:
        s = g.seq_of(cell)
        before = g.text[cell - 1]
        if kind == DEL:
            ref_a, alt_a = before + g.text[cell:cell + length], before
        else:
            ref_a, alt_a = before, before + S
        info = "TYPE=%s;LEN=%d;SF=%d;SR=%d;RS=%d;AF=%s" % ("DEL" if kind == DEL else "INS", length, fwd, rev, rs, af_text(fwd + rev, rs))
        out.append("\t".join([g.names[s], str(cell - g.first[s]), ".", ref_a, alt_a, ".", "PASS", info]))
    return "".join(line + "\n" for line in out)
