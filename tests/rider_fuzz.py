"""Random cases for the passes that ride on a sample's records: --indels, --linkage, --codons, --haplotypes, --read-pileup and the row store
they share, with and without --adapter, --primers and --min-base-qual in front of them.

make_case(seed, iteration) draws one case -- k, a genome, reads, every parameter, the sites and regions, how the sample is pushed --
from numpy's generator seeded with (seed, iteration), and the read pileup's end distance and place among the other counts from a
second one seeded with (seed, iteration, 1); nothing else goes in.  make_case(seed, iteration, trim=True) is the same base case with
adapters and primers drawn from the second generator and reads that carry them.  expected(case) is what the restatements
(tests/indels_ref.py, linkage_ref.py, codons_ref.py, haplotypes_ref.py, read_pileup_ref.py; adapter_ref.py and primer_ref.py for the
reads as the rule sees them) make of it; nothing of the product is asked.  check_host holds the host twins (bronko_amd.hostlib) against
that, check_engine the engine.  tally() counts what a run of cases has exercised, for the conditions of tests/test_rider_fuzz_cpu.py.
tests/test_gpu_rider_fuzz.py and tools/fuzz_riders.py run the same cases.

The generator itself is plain Python and numpy; the product is imported by the two check functions only.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import adapter_ref, codons_ref, haplotypes_ref, indels_ref, linkage_ref, read_pileup_ref

B = "ACGT"
KS = (11, 15, 19, 21, 21, 25, 31, 31)            # 21 and 31 twice as likely
PUSHES = ("packed", "packed_ends", "ascii", "ascii_device", "ascii_qual")
THRESHOLDS = ((1, 0), (1, 1000000), (2, 0), (5, 30000), (2, 500000))
MIN_QUAL = 20
LDS_PAIRS = 512                                  # kLinkLdsPairs: a counter table of more pairs takes the global path
SEED = 20261                                     # the suite's seed
BLOCK, BLOCKS = 30, 4                            # the suite's iterations: BLOCKS blocks of BLOCK
TRIM_BLOCKS = 2                                  # ... and TRIM_BLOCKS blocks of BLOCK with adapters and primers set
MERGE_ROUNDS = 4                                 # kMergeRounds: a wave merges at most so many groups of equal adds
FINISH_BLOCK = 1024                              # kPileFinishBlock: a genome of fewer cells leaves finish threads without a cell


def rand_seq(rng, n: int) -> str:
    return "".join(B[i] for i in rng.integers(0, 4, n))


def make_genome(rng, n: int):
    """(letters, whether a reverse-complement repeat was laid): random letters, direct and reverse-complement repeats of 15 to 120
    bases, a homopolymer or dinucleotide stretch"""
    g = list(rand_seq(rng, n))
    rc_repeat = False
    for _ in range(int(rng.integers(0, 4))):
        ln = int(rng.integers(15, 121))
        a, b = int(rng.integers(0, n - ln)), int(rng.integers(0, n - ln))
        seg = "".join(g[a:a + ln])
        if rng.random() < 0.5:
            seg, rc_repeat = indels_ref.revcomp(seg), True
        g[b:b + ln] = seg
    if rng.random() < 0.4:
        ln = int(rng.integers(10, 60))
        a = int(rng.integers(0, n - ln))
        unit = rand_seq(rng, int(rng.integers(1, 3)))
        g[a:a + ln] = (unit * ln)[:ln]
    return "".join(g), rc_repeat


@dataclass
class Case:
    seed: int
    it: int
    k: int
    names: list
    seqs: list                       # letters, N runs included
    reads: list                      # bytes, as pushed
    quals: list                      # bytes, one line per read (used by ascii_qual only)
    kinds: dict                      # how many reads of each kind were drawn
    link_M: int
    indel_L: int
    indel_M: int
    min_reads: int
    min_af_ppm: int
    initial_rows: int
    table_log2: int
    sites: list
    max_dist: int
    codon_regions: list
    hap_regions: list
    push: str
    batch: int | None
    n_mates: int
    twice: bool
    linkage_first: bool
    rc_repeat: bool
    n_run: tuple | None              # (first cell, length)
    first: list = field(default_factory=list)
    # drawn from the second generator, (seed, it, 1): the read pileup's first end distance, where among the other counts it is taken
    # (0 before linkage, 1 between codons and haplotypes, 2 last), which row and which d make the second end distance, what is
    # downloaded once more at the end
    pile_end: int = 10
    pile_at: int = 2
    pile_row: float = 0.0
    pile_d: int = 0
    recheck: str = "pairs"
    # a trimmed case: the adapters and primers the engine is given (the reads carry them)
    trim: bool = False
    adapters: list = field(default_factory=list)
    min_overlap: int = 5
    max_error_rate: float = 0.1
    primers: list = field(default_factory=list)
    primer_m: int = 1
    _seen: tuple | None = None

    def files(self):
        return [("fuzz", [(name, s.encode()) for name, s in zip(self.names, self.seqs)])]

    def genome(self) -> indels_ref.Genome:
        return indels_ref.Genome(list(self.names), list(self.seqs), self.k)

    def mates(self) -> list:
        n = len(self.reads)
        return [(0, n)] if self.n_mates == 1 else [(0, n // 2), (n // 2, n)]

    def _see(self) -> tuple:
        if self._seen is None:
            min_qual = MIN_QUAL if self.push == "ascii_qual" else 0
            if not self.trim:
                self._seen = ([r.decode() for r in adapter_ref.masked(self.reads, self.quals, min_qual)], None)
            else:                                                  # truncate, then mask, then substitute; the counters are a mate's
                seen, counts = [], []
                for lo, hi in self.mates():
                    want, ac, pc, _ = adapter_ref.seen_reads(self.reads[lo:hi], self.quals[lo:hi], self.adapters, self.min_overlap, self.max_error_rate, self.k,
                                                             min_qual, self.primers, self.primer_m)
                    seen += [r.decode() for r in want]
                    counts.append((ac, pc))
                self._seen = (seen, counts)
        return self._seen

    def reads_seen(self) -> list:
        """The reads as the rule sees them: under ascii_qual a base whose quality is below MIN_QUAL is an N; in a trimmed case cut at
        the adapter first and with the primers' letters written as N last (adapter_ref.seen_reads)"""
        return self._see()[0]

    def trim_counts(self):
        """[(bk_adapter_stats, bk_primer_stats) per mate] of a trimmed case, None of another"""
        return self._see()[1]

    def describe(self) -> str:
        return ("seed=%d it=%d k=%d seqs=%s n_run=%s rc_repeat=%d reads=%d kinds=%s link_M=%d indel_L=%d indel_M=%d min_reads=%d ppm=%d initial_rows=%d "
                "table_log2=%d sites=%d max_dist=%d codon_regions=%d hap_regions=%d push=%s batch=%s mates=%d twice=%d linkage_first=%d "
                "pile_end=%d pile_at=%d pile_row=%.4f pile_d=%d recheck=%s trim=%d adapters=%s O=%d E=%g primers=%s m=%d" %
                (self.seed, self.it, self.k, [len(s) for s in self.seqs], self.n_run, self.rc_repeat, len(self.reads),
                 ",".join("%s:%d" % kv for kv in sorted(self.kinds.items())), self.link_M, self.indel_L, self.indel_M, self.min_reads, self.min_af_ppm,
                 self.initial_rows, self.table_log2, len(self.sites), self.max_dist, len(self.codon_regions), len(self.hap_regions), self.push, self.batch,
                 self.n_mates, self.twice, self.linkage_first, self.pile_end, self.pile_at, self.pile_row, self.pile_d, self.recheck, self.trim,
                 [len(a) for a in self.adapters], self.min_overlap, self.max_error_rate, [len(p) for p in self.primers], self.primer_m))


def _cut(rng, text: str, k: int) -> list:
    """The genome cut into one to three sequences; a cut is often less than k or less than 2k from an end or from another cut"""
    n = len(text)
    cuts = {0, n}
    for _ in range(int(rng.choice([0, 0, 1, 1, 2]))):
        u = rng.random()
        at = sorted(cuts)[int(rng.integers(0, len(cuts)))]
        d = int(rng.integers(1, k)) if u < 0.25 else int(rng.integers(k, 2 * k)) if u < 0.5 else int(rng.integers(1, n))
        c = at + d if at + d < n else at - d
        if 0 < c < n:
            cuts.add(c)
    cuts = sorted(cuts)
    return [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _regions(rng, seqs, first, n_run, spans, limits: tuple, per: int, n_max: int = 40) -> list:
    """0 to n_max regions (first cell, units) of `per` cells a unit and at most one of `limits` units, each inside one sequence:
    anywhere, ending at a sequence's last cell, over the N run, nested in or equal to an earlier one, inside the stretch of cells that
    one of the reads was drawn from (`spans`: so that rows span regions at any depth of cover)"""
    out = []
    fit = [s for s in range(len(seqs)) if len(seqs[s]) >= per]
    if not fit:
        return out
    for _ in range(int(rng.integers(0, n_max + 1))):
        u, longest = rng.random(), int(rng.choice(limits))
        if u < 0.15 and out:                                       # nested in or equal to an earlier one
            c0, units = out[int(rng.integers(0, len(out)))]
            skip = int(rng.integers(0, units))
            units = int(rng.integers(1, units - skip + 1)) if rng.random() < 0.7 else units - skip
            out.append((c0 + per * skip, units))
            continue
        s = fit[int(rng.integers(0, len(fit)))]
        lo, hi = first[s], first[s] + len(seqs[s])
        if u < 0.35 and n_run is not None and any(first[q] <= n_run[0] < first[q] + len(seqs[q]) for q in fit):   # over the N run
            s = [q for q in fit if first[q] <= n_run[0] < first[q] + len(seqs[q])][0]
            lo, hi = first[s], first[s] + len(seqs[s])
            c0 = max(lo, min(n_run[0] - int(rng.integers(0, 3 * per + 1)), hi - per))
            units = int(rng.integers(1, min(longest, (hi - c0) // per) + 1))
        elif u < 0.7 and spans and rng.random() < 0.6:             # inside the stretch a read was drawn from
            a, ln = spans[int(rng.integers(0, len(spans)))]
            s = max(q for q in range(len(seqs)) if first[q] <= a)
            lo, hi = max(a, first[s]), min(a + ln, first[s] + len(seqs[s]))
            if hi - lo < per:
                continue
            c0 = int(rng.integers(lo, hi - per + 1))
            units = int(rng.integers(1, min(longest, (hi - c0) // per) + 1))
        elif u < 0.5:                                              # ends at the sequence's last cell
            units = int(rng.integers(1, min(longest, (hi - lo) // per) + 1))
            c0 = hi - per * units
        else:
            c0 = int(rng.integers(lo, hi - per + 1))
            units = int(rng.integers(1, min(longest, (hi - c0) // per) + 1))
        out.append((c0, units))
    return out


def _errors(rng, letters: list, positions) -> None:
    for p in positions:
        if letters[p] in B:
            letters[p] = B[(B.index(letters[p]) + int(rng.integers(1, 4))) & 3]


def _trim(rng, case: Case, src: str) -> None:
    """Adapters and primers for the case, and reads that carry them.  One to three adapters of the two presets and a random 12 to
    30-mer; one to six primers of 18 to 30 bases cut from either strand of the genome, clear of the N run; only what bk_adapters_set
    and bk_primers_set accept.  About 20 % of the reads are drawn again to begin at a primer and about 10 % to end at the reverse
    complement of one, with up to primer_m + 1 errors in it; then about 30 % of the reads of more than 50 bases run into an adapter
    with up to two errors and a tail -- at a drawn position, or right behind the reverse-complemented primer."""
    n = len(src)
    pool = [adapter_ref.PRESETS["truseq"], adapter_ref.PRESETS["nextera"], rand_seq(rng, int(rng.integers(12, 31))).encode()]
    case.adapters = [pool[int(i)] for i in rng.permutation(3)[:int(rng.integers(1, 4))]]
    case.min_overlap = int(rng.choice([3, 5, 12]))
    case.max_error_rate = float(rng.choice([0.0, 0.1, 0.2]))
    case.primer_m = int(rng.choice([0, 1, 2]))
    sites = []                                                     # (first cell, length, whether the primer is the reverse strand's)
    for _ in range(int(rng.integers(1, 7))):
        L = int(rng.integers(18, 31))
        before = 0 if case.n_run is None else max(0, case.n_run[0] - L + 1)          # starts that end in front of the N run
        after = n - L + 1 if case.n_run is None else max(0, n - L + 1 - (case.n_run[0] + case.n_run[1]))
        a = int(rng.integers(0, before + after))
        if a >= before and case.n_run is not None:
            a = a - before + case.n_run[0] + case.n_run[1]
        sites.append((a, L, bool(rng.random() < 0.5)))
    case.primers = [(indels_ref.revcomp(src[a:a + L]) if rev else src[a:a + L]).encode() for a, L, rev in sites]
    for i in range(len(case.reads)):
        r, u, kind = case.reads[i].decode(), rng.random(), None
        if u < 0.3:
            a, L, rev = sites[int(rng.integers(0, len(sites)))]
            ln = max(len(r), L)
            s = list(indels_ref.revcomp(src[max(0, a + L - ln):a + L]) if rev else src[a:a + ln])   # begins with the primer
            _errors(rng, s, rng.choice(L, size=int(rng.integers(0, case.primer_m + 2)), replace=False))
            if rng.random() < 0.5:
                _errors(rng, s, [p for p in np.nonzero(rng.random(len(s)) < 0.01)[0] if p >= L])
            r, kind = "".join(s), "at_primer"
            if u >= 0.2:
                r, kind = indels_ref.revcomp(r), "to_primer"
        if len(r) > 50 and rng.random() < 0.3:
            A = list(case.adapters[int(rng.integers(0, len(case.adapters)))].decode())
            _errors(rng, A, rng.choice(len(A), size=int(rng.integers(0, 3)), replace=False))
            tail = "G" * len(r) if rng.random() < 0.5 else rand_seq(rng, len(r))
            if kind == "to_primer" and rng.random() < 0.5:         # a short amplicon read through: primer, adapter, tail
                r = r + "".join(A) + tail[:int(rng.integers(0, 21))]
            else:
                r = (r[:int(rng.integers(0, len(r) + 1))] + "".join(A) + tail)[:len(r)]
            kind = (kind + "+adapter") if kind else "adapter"
        if kind is not None:
            qv = rng.integers(30, 41, len(r))
            qv[rng.random(len(r)) < 0.01] = 7
            case.reads[i], case.quals[i] = r.encode(), (qv + 33).astype(np.uint8).tobytes()
            case.kinds[kind] = case.kinds.get(kind, 0) + 1
    case.trim = True


def make_case(seed: int, it: int, trim: bool = False) -> Case | None:
    """Case `it` of `seed`, or None where no sequence holds a k-mer (no index is built of those).  What the first generator draws is
    the case as it was before the read pileup and the trimming joined: everything of those comes from a second generator, so that an
    iteration's genome, reads and parameters stay what they were.  With `trim` the second generator also draws adapters and primers
    and rewrites some of the reads to carry them (_trim)."""
    rng = np.random.default_rng([seed, it])
    k = int(rng.choice(KS))
    text, rc_repeat = make_genome(rng, int(rng.integers(300, 6001)))
    seqs = _cut(rng, text, k)
    first = [0]
    for s in seqs[:-1]:
        first.append(first[-1] + len(s))
    n_run = None
    if rng.random() < 0.4:                                         # a run of N; one time in four at a sequence's first or last cell
        ln = int(rng.integers(1, 31))
        fit = [s for s in range(len(seqs)) if len(seqs[s]) >= ln]
        if fit:
            s = fit[int(rng.integers(0, len(fit)))]
            u = rng.random()
            at = 0 if u < 0.125 else len(seqs[s]) - ln if u < 0.25 else int(rng.integers(0, len(seqs[s]) - ln + 1))
            seqs[s] = seqs[s][:at] + "N" * ln + seqs[s][at + ln:]
            n_run = (first[s] + at, ln)
    if all(len(s) < k for s in seqs):
        return None
    # the reads are drawn from the genome with letters in the N run's place: a record may lie over the run
    src = "".join(seqs)
    if n_run is not None:
        src = src[:n_run[0]] + rand_seq(rng, n_run[1]) + src[n_run[0] + n_run[1]:]
    n = len(src)
    forced = (2 * k - 1, 2 * k, 159, 160, 161, 255, 256, 257)
    reads, quals, kinds, spans = [], [], {}, []
    amplicons = []
    if rng.random() < 0.35:
        for _ in range(int(rng.integers(1, 4))):
            ln = min(n, int(rng.integers(2 * k, 301)))
            amplicons.append((int(rng.integers(0, n - ln + 1)), ln))
    for _ in range(int(rng.integers(1, 401))):
        u = rng.random()
        ln = int(rng.choice(forced)) if u < 0.2 else int(rng.integers(20, 201)) if u < 0.65 else int(rng.integers(20, 601))
        ln = min(ln, n)
        a = int(rng.integers(0, n - ln + 1))
        if amplicons and rng.random() < 0.6:                       # ... or one of the case's amplicons: many records of one stretch
            a, ln = amplicons[int(rng.integers(0, len(amplicons)))]
        r = src[a:a + ln]
        u = rng.random()
        kind = "plain"
        if u < 0.08:
            kind, r = "foreign", rand_seq(rng, ln)
            if rng.random() < 0.4 and ln > 30:                     # ... with a stretch of the reference spliced in
                kind, q = "foreign_spliced", int(rng.integers(0, ln - 25))
                r = r[:q] + src[a + q:a + q + 25] + r[q + 25:]
        elif u < 0.15 and ln > 60:
            kind, b2 = "chimera", int(rng.integers(0, n - ln + 1))
            r = r[:ln // 2] + src[b2 + ln // 2:b2 + ln]
        elif u < 0.55 and ln > 40:                                 # an indel of 1 to 33 bases; 31, 32 and 33 often
            d = int(rng.choice([31, 32, 33])) if rng.random() < 0.25 else int(rng.integers(1, 34))
            p = int(rng.integers(10, ln - 9))
            if rng.random() < 0.5:
                kind, r = "deletion", r[:p] + src[a + p + d:a + ln + d]
            else:
                kind, r = "insertion", (r[:p] + rand_seq(rng, d) + r[p:])[:max(ln, 20)]
        rate = float(rng.choice([0.0, 0.005, 0.02, 0.05]))
        r = list(r)
        for p in np.nonzero(rng.random(len(r)) < rate)[0]:
            r[p] = B[(B.index(r[p]) + int(rng.integers(1, 4))) & 3]
        if rng.random() < 0.02:
            r[int(rng.integers(0, len(r)))] = "N"
        r = "".join(r)
        if len(r) < 20:
            r = r + rand_seq(rng, 20 - len(r))
        if rng.random() < 0.5:
            r = "".join({"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}[c] for c in reversed(r))
        qv = rng.integers(30, 41, len(r))
        qv[rng.random(len(r)) < 0.01] = 7
        reads.append(r.encode())
        quals.append((qv + 33).astype(np.uint8).tobytes())
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == "plain":
            spans.append((a, ln))
    min_reads, min_af_ppm = THRESHOLDS[int(rng.integers(0, len(THRESHOLDS)))]
    max_dist = int(rng.choice([1, 2, 150, 1000, 65519]))
    sites = set(int(c) for c in rng.integers(0, n, int(rng.integers(0, 80))))
    if rng.random() < 0.3:                                         # a dense run: more than LDS_PAIRS pairs at any max_dist
        s = max(range(len(seqs)), key=lambda q: len(seqs[q]))
        ln = min(len(seqs[s]), int(rng.integers(60, 121)) if max_dist >= 150 else 560 // max_dist + int(rng.integers(20, 60)))
        at = first[s] + int(rng.integers(0, len(seqs[s]) - ln + 1))
        sites |= set(range(at, at + ln))
    case = Case(seed=seed, it=it, k=k, names=["s%d" % i for i in range(len(seqs))], seqs=seqs, reads=reads, quals=quals, kinds=kinds,
                link_M=int(rng.choice([0, 2, 8])), indel_L=int(rng.choice([1, 8, 32])), indel_M=int(rng.choice([0, 2, 8])),
                min_reads=min_reads, min_af_ppm=min_af_ppm, initial_rows=int(rng.choice([1, 16, 65536])), table_log2=10,
                sites=sorted(sites), max_dist=max_dist,
                codon_regions=_regions(rng, seqs, first, n_run, spans, (10, 40, 120), 3), hap_regions=_regions(rng, seqs, first, n_run, spans, (20, 20, 60, 60, 150, 600), 1),
                push=PUSHES[int(rng.integers(0, len(PUSHES)))], batch=int(rng.integers(1, 501)) if rng.random() < 0.4 else None,
                n_mates=2 if rng.random() < 0.3 and len(reads) > 1 else 1, twice=bool(rng.random() < 0.3), linkage_first=bool(rng.random() < 0.2),
                rc_repeat=rc_repeat, n_run=n_run, first=first)
    rng2 = np.random.default_rng([seed, it, 1])
    case.pile_end = int((0, 1, 10, k, 80, 128, 255)[int(rng2.integers(0, 7))])
    case.pile_at = int(rng2.integers(0, 3))
    case.pile_row = float(rng2.random())
    case.pile_d = int(rng2.integers(-1, 2))
    case.recheck = ("pairs", "codons")[int(rng2.integers(0, 2))]
    if trim:
        _trim(rng2, case, src)
    return case


@dataclass
class Expected:
    g: indels_ref.Genome
    indels: indels_ref.Result
    rows: list
    tallies: dict
    pairs: list
    codons: np.ndarray
    hap: tuple                       # (cover, ref_count, entries)
    ends: tuple = ()                 # the two end distances of the read pileup: the drawn one, and about half the length of a drawn row
    pile: dict = field(default_factory=dict)          # {E: the (cells, 12) counters}
    pile_summary: dict = field(default_factory=dict)  # {E: (covered, bases)}
    trim_counts: list | None = None  # [(adapter counters, primer counters) per mate] of a trimmed case


def expected(case: Case) -> Expected:
    """The restatements' results of the case; case.table_log2 is raised where the events do not fit 2^10 slots"""
    g = case.genome()
    seen = case.reads_seen()
    ind = indels_ref.indel_events(g, seen, case.indel_L, case.indel_M)
    while len(ind.events) > 1 << case.table_log2:
        case.table_log2 += 1
    rows, t = linkage_ref.link_rows(g, seen, case.link_M)
    pairs = linkage_ref.link_count(g, rows, case.sites, case.max_dist)
    exp = Expected(g, ind, rows, t, pairs, codons_ref.codon_count(g, rows, case.codon_regions), haplotypes_ref.hap_count(g, rows, case.hap_regions))
    # the second end distance puts a row at n = 2E - 1, 2E or 2E + 1: the count kernel takes its two ways apart at n <= 2E
    second = case.pile_end
    if rows:
        second = min(read_pileup_ref.MAX_END, (rows[int(case.pile_row * len(rows))][1] + case.pile_d) // 2)
    exp.ends = (case.pile_end, second)
    for E in exp.ends:
        if E not in exp.pile:
            exp.pile[E] = read_pileup_ref.read_pileup(g, rows, E)
            exp.pile_summary[E] = read_pileup_ref.summary(exp.pile[E], rows)
    exp.trim_counts = case.trim_counts()
    return exp


def tally(case: Case, exp: Expected, into: dict) -> dict:
    """What the case exercised, from the restatements' results alone, added into `into`"""
    def add(name, v=1):
        into[name] = into.get(name, 0) + int(v)
    t = exp.tallies
    add("iterations")
    add("k=%d" % case.k)
    add("placed", t["placed"])
    add("placed_fwd", sum(1 for r in exp.rows if r[2] == 0))
    add("placed_rev", sum(1 for r in exp.rows if r[2] == 1))
    add("discordant", t["discordant"])
    add("unplaced", t["unplaced"])
    add("rows_8_mismatches", sum(1 for r in exp.rows if len(r[3]) == 8))
    add("events", len(exp.indels.events))
    add("deletions", sum(1 for e in exp.indels.events if e[1] == indels_ref.DEL))
    add("insertions", sum(1 for e in exp.indels.events if e[1] == indels_ref.INS))
    # a record that max_len turned away: alone, with no limit on the length and on the mismatches, it supports an event longer than max_len
    # (the length is the first thing the rule looks at once the anchors stand)
    lone, away = indels_ref.new_result(exp.g), 0
    records = [rec for read in case.reads_seen() for rec in indels_ref.records_of(read, case.k)]
    for rec in records:
        lone.events.clear()
        indels_ref.add_record(exp.g, rec, 1 << 30, 1 << 30, lone)
        away += any(e[2] > case.indel_L for e in lone.events)
    add("max_len_turned_away", away)
    add("it_several_sequences", len(case.seqs) > 1)
    add("it_n_run", case.n_run is not None)
    add("it_n_run_at_an_end", case.n_run is not None and any(case.n_run[0] == f or case.n_run[0] + case.n_run[1] == f + len(s) for f, s in zip(case.first, case.seqs)))
    add("it_rc_repeat", case.rc_repeat)
    add("it_global_pairs", len(exp.pairs) > LDS_PAIRS)
    add("it_record_over_300", any(len(r) > 300 for r in records))
    add("it_seq_under_k", any(len(s) < case.k for s in case.seqs))
    add("it_seq_under_2k", any(case.k <= len(s) < 2 * case.k for s in case.seqs))
    add("it_hap_table_full", len(exp.hap[2]) > 1024)
    add("codon_counts", int(exp.codons.sum()))
    add("hap_entries", len(exp.hap[2]))
    add("hap_cover", sum(exp.hap[0]))
    add("hap_cover_with_a_list", sum(exp.hap[0]) - sum(exp.hap[1]))
    add("pair_counts", sum(sum(c) for _, _, c in exp.pairs))
    # the read pileup, per end distance the case counts at
    for E in exp.ends:
        add("pile_rows_whole", sum(1 for r in exp.rows if r[1] <= 2 * E))
        add("pile_rows_split", sum(1 for r in exp.rows if r[1] > 2 * E))
        add("pile_rows_at_2e", sum(1 for r in exp.rows if 2 * E - 1 <= r[1] <= 2 * E + 1))
        add("pile_subs_near", sum(1 for r in exp.rows for off, _ in r[3] if min(off, r[1] - 1 - off) < E))
        add("pile_subs_far", sum(1 for r in exp.rows for off, _ in r[3] if min(off, r[1] - 1 - off) >= E))
        add("pile_near_counts", int(exp.pile[E][:, 8:].sum()))
    add("it_pile_end_0", 0 in exp.ends)
    add("it_pile_end_255", 255 in exp.ends)
    add("it_pile_at_%d" % case.pile_at)
    add("it_under_1024_cells", exp.g.cells < FINISH_BLOCK)
    # 64-row chunks of the restatement's sorted rows in which more than MERGE_ROUNDS groups of two or more rows share (strand, cell0):
    # a wave of those runs out of merge rounds.  The store's order on the device need not be the restatement's, so this is an
    # indication and no guarantee; tests/test_gpu_read_pileup_waves.py fixes the composition of a wave.
    for at in range(0, len(exp.rows), 64):
        groups = {}
        for r in exp.rows[at:at + 64]:
            groups[(r[2], r[0])] = groups.get((r[2], r[0]), 0) + 1
        add("pile_waves")
        add("pile_waves_over_4_groups", sum(1 for v in groups.values() if v > 1) > MERGE_ROUNDS)
    if case.trim:
        records = lambda reads: sum(len(indels_ref.records_of(r, case.k)) for r in reads)
        for (lo, hi), (ac, pc) in zip(case.mates(), exp.trim_counts):
            add("trim_reads_cut", ac[0])
            add("trim_bases_removed", ac[1])
            add("trim_5", pc[0])
            add("trim_3", pc[1])
            add("trim_bases_masked", pc[2])
        # a read that held a record and holds none as the rule sees it: emptied, or shortened below k
        min_qual = MIN_QUAL if case.push == "ascii_qual" else 0
        plain = [r.decode() for r in adapter_ref.masked(case.reads, case.quals, min_qual)]
        add("trim_reads_emptied", sum(1 for a, b in zip(plain, case.reads_seen()) if records([a]) > 0 and records([b]) == 0))
    return into


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _differ(got, want):
    return [x for x in got if x not in want][:3], [x for x in want if x not in got][:3]


def _indel_counters(c):
    return (c["records"], c["anchored"], c["ref_spanning"], c["supporting"], c["discordant"])


def _report_rows(g, res, min_reads, ppm):
    return [(c, ln if kd == indels_ref.DEL else -ln, f, r, rs, indels_ref.seq_code(s)) for c, kd, ln, s, f, r, rs in indels_ref.report(g, res, min_reads, ppm)]


def _span(exp):
    return np.array(exp.indels.span_sums()[:exp.g.cells], np.int64).astype(np.uint32)


def _pile_differs(got, want):
    return np.argwhere(np.asarray(got) != want)[:5].tolist()


def check_host(case: Case, exp: Expected) -> None:
    """The host twins on the case (on the reads as the rule sees them) against the restatements; AssertionError names what differs"""
    from bronko_amd import hostlib
    from bronko_amd.engine import link_rows as decode_rows
    ix = hostlib.HostIndex.build_mem(case.k, case.files())
    try:
        seen = case.reads_seen()
        rows, span, counters = hostlib.indel_events(ix, 0, seen, case.indel_L, case.indel_M)
        want = indels_ref.table_rows(exp.g, exp.indels)
        assert rows == want, ("indel events",) + _differ(rows, want)
        assert np.array_equal(span, _span(exp)), ("indel span", np.flatnonzero(span != _span(exp))[:5])
        assert counters == _indel_counters(exp.indels.counters), ("indel counters", counters, exp.indels.counters)
        raw, lc = hostlib.link_rows(ix, 0, seen, case.link_M)
        got = decode_rows(raw)
        assert got == exp.rows, ("rows",) + _differ(got, exp.rows)
        t = exp.tallies
        assert lc == (t["records"], t["placed"], t["unplaced"], t["discordant"]), ("link tallies", lc, t)
        got = hostlib.link_count(ix, 0, raw, case.sites, case.max_dist)
        assert got == exp.pairs, ("pairs", len(got), len(exp.pairs), [x for x in zip(got, exp.pairs) if x[0] != x[1]][:2])
        if case.codon_regions:
            got = hostlib.codon_count(ix, 0, raw, case.codon_regions)
            assert np.array_equal(got, exp.codons), ("codons", np.argwhere(got != exp.codons)[:5].tolist())
        cover, ref, entries = hostlib.hap_count(ix, 0, raw, case.hap_regions)
        assert (list(cover), list(ref)) == (exp.hap[0], exp.hap[1]), "haplotype cover / ref_count"
        assert entries == exp.hap[2], ("haplotype entries",) + _differ(entries, exp.hap[2])
        for E in exp.ends:
            got = hostlib.read_pileup_count(ix, 0, raw, E)
            assert got.shape == exp.pile[E].shape and np.array_equal(got, exp.pile[E]), ("read pileup", E, _pile_differs(got, exp.pile[E]))
    finally:
        ix.close()


def _push(eng, case: Case, mate: int, a: int, b: int, keep: list) -> None:
    from bronko_amd import pack_reads, pack_reads_ends
    reads = case.reads[a:b]
    if case.push == "packed" and not case.trim:                     # (the push without end flags is refused once primers are set)
        w, l = pack_reads(reads, case.k)
        eng.push_reads(mate, w, l)
    elif case.push in ("packed", "packed_ends"):
        w, l, e = pack_reads_ends(reads, case.k)
        eng.push_reads_ends(mate, w, l, e)
    elif case.push == "ascii":
        eng.push_reads_ascii(mate, reads)
    elif case.push == "ascii_qual":
        eng.push_reads_ascii(mate, reads, case.quals[a:b], MIN_QUAL)
    else:
        import torch
        flat = np.frombuffer(b"".join(reads), np.uint8)
        off = np.zeros(len(reads) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        d_b = torch.from_numpy(np.concatenate([flat, np.zeros(64, np.uint8)])).to("cuda:0")
        d_off = torch.from_numpy(off).to("cuda:0")
        torch.cuda.synchronize()
        keep += [d_b, d_off]                                       # (alive until the sample is finalized)
        eng.push_reads_ascii_device(mate, d_b.data_ptr(), d_off.data_ptr(), len(reads), int(off[-1]), max(len(r) for r in reads))


def _sample(eng, case: Case) -> None:
    eng.sample_begin()
    keep = []
    for m, (lo, hi) in enumerate(case.mates()):
        step = case.batch or max(1, hi - lo)
        for a in range(lo, hi, step):
            _push(eng, case, m, a, min(hi, a + step), keep)
    eng.sample_finalize(case.n_mates)


def _check_pile(eng, exp: Expected, E: int, what: str) -> None:
    """One read-pileup count of the finalized sample at end distance E: every counter of every cell and every field of the summary"""
    eng.sample_read_pileup(E)
    summ, cells = eng.download_read_pileup()
    want = exp.pile[E]
    assert cells.shape == want.shape and np.array_equal(cells, want), ("read pileup " + what, E, _pile_differs(cells, want))
    got = (summ.rows, summ.n_cells, summ.end_dist, summ.covered, summ.bases)
    assert got == (exp.tallies["placed"], exp.g.cells, E) + exp.pile_summary[E], ("read pileup summary " + what, E, got, exp.pile_summary[E])


def _check_sample(eng, case: Case, exp: Expected) -> None:
    from bronko_amd import BronkoError
    g, c = exp.g, exp.indels.counters
    if case.trim:
        for m, (ac, pc) in enumerate(exp.trim_counts):
            got = (eng.adapter_stats(m), eng.primer_stats(m))
            assert got == (ac, pc), ("trimming counters of mate %d" % m, got, (ac, pc))
    # indels: the reported records at the drawn thresholds, the whole table, the span, the summary
    eng.sample_indels(case.min_reads, case.min_af_ppm)
    summ, rows = eng.download_indels()
    want = _report_rows(g, exp.indels, case.min_reads, case.min_af_ppm)
    assert rows == want, ("reported indels",) + _differ(rows, want)
    assert (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.discordant) == _indel_counters(c), ("indel counters", c)
    assert (summ.candidates, summ.reported, summ.overflow) == (len(exp.indels.events), len(want), 0), ("indel summary", summ.candidates, summ.reported)
    eng.sample_indels(1, 0)
    summ, rows = eng.download_indels()
    want = indels_ref.table_rows(g, exp.indels)
    assert rows == want, ("indel table",) + _differ(rows, want)
    assert summ.candidates == summ.reported == len(want)
    span = eng.download_indel_span()
    assert np.array_equal(span, _span(exp)), ("indel span", np.flatnonzero(span != _span(exp))[:5])
    # linkage: the rows, the tallies, every pair
    got = eng.download_link_rows()
    assert got == exp.rows, ("rows", len(got), len(exp.rows)) + _differ(got, exp.rows)
    if case.pile_at == 0:
        _check_pile(eng, exp, exp.ends[0], "before linkage")
    eng.sample_linkage(case.sites, case.max_dist)
    summ, pairs = eng.download_linkage()
    t = exp.tallies
    assert (summ.records, summ.placed, summ.unplaced, summ.discordant) == (t["records"], t["placed"], t["unplaced"], t["discordant"]), ("link tallies", t)
    assert (summ.n_sites, summ.max_dist, summ.n_pairs) == (len(case.sites), case.max_dist, len(exp.pairs)), ("link summary", summ.n_pairs, len(exp.pairs))
    assert pairs == exp.pairs, ("pairs", [x for x in zip(pairs, exp.pairs) if x[0] != x[1]][:2])
    # codons
    eng.sample_codons(case.codon_regions)
    summ, counts = eng.download_codons()
    assert (summ.rows, summ.n_codons, summ.n_regions) == (t["placed"], len(exp.codons), len(case.codon_regions)), "codon summary"
    assert np.array_equal(counts, exp.codons), ("codons", np.argwhere(counts != exp.codons)[:5].tolist())
    if case.pile_at == 1:
        _check_pile(eng, exp, exp.ends[0], "between codons and haplotypes")
    # haplotypes: a table of 2^10 slots; where it cannot hold every haplotype the hot counters stay exact, and 2^16 slots hold all
    cover, ref, entries = exp.hap
    log2 = 10
    eng.sample_haplotypes(case.hap_regions, log2)
    if len(entries) > 1 << log2:
        try:
            eng.download_haplotypes()
            raise AssertionError("a table of 2^10 slots held %d haplotypes" % len(entries))
        except BronkoError as err:
            assert err.status == -6, err
            summ, cv, rf = err.hap
            assert summ.dropped > 0 and (summ.rows, summ.n_regions, summ.table_log2) == (t["placed"], len(case.hap_regions), log2)
            assert (list(cv), list(rf)) == (cover, ref), "haplotype cover / ref_count of a full table"
        log2 = 16
        eng.sample_haplotypes(case.hap_regions, log2)
    summ, cv, rf, got = eng.download_haplotypes()
    assert (summ.rows, summ.n_regions, summ.table_log2, summ.dropped, summ.entries) == (t["placed"], len(case.hap_regions), log2, 0, len(entries)), \
        ("haplotype summary", summ.rows, summ.dropped, summ.entries, len(entries))
    assert (list(cv), list(rf)) == (cover, ref), "haplotype cover / ref_count"
    assert got == entries, ("haplotype entries",) + _differ(got, entries)
    # the read pileup where it was not counted yet, then at the second end distance; a count in between left its neighbours' results alone
    if case.pile_at == 2:
        _check_pile(eng, exp, exp.ends[0], "last")
    _check_pile(eng, exp, exp.ends[1], "at the second end distance")
    if case.recheck == "codons" and case.codon_regions:
        counts = eng.download_codons()[1]
        assert np.array_equal(counts, exp.codons), ("codons after the read pileup", np.argwhere(counts != exp.codons)[:5].tolist())
    else:
        pairs = eng.download_linkage()[1]
        assert pairs == exp.pairs, ("pairs after the read pileup", [x for x in zip(pairs, exp.pairs) if x[0] != x[1]][:2])


def check_engine(case: Case, exp: Expected) -> None:
    """One engine for the case: create, enable, sample (twice where the case says so), every download, close"""
    from bronko_amd.hostlib import HostIndex
    ix = HostIndex.build_mem(case.k, case.files())
    eng = None
    try:
        eng = ix.engine()
        enable = [lambda: eng.indels_enable(case.indel_L, case.indel_M, case.table_log2), lambda: eng.linkage_enable(case.link_M, case.initial_rows)]
        for fn in (enable[::-1] if case.linkage_first else enable):
            fn()
        if case.trim:
            eng.adapters_set(case.adapters, case.min_overlap, case.max_error_rate)
            eng.primers_set(case.primers, case.primer_m)
        for _ in range(2 if case.twice else 1):
            _sample(eng, case)
            _check_sample(eng, case, exp)
    finally:
        if eng is not None:
            eng.close()
        ix.close()


def run(seed: int, first: int, count: int, check, verbose: bool = False, out=print, trim: bool = False) -> tuple:
    """Cases first .. first + count - 1 of `seed`, trimmed ones with `trim`, through `check` (check_host or check_engine): (cases run,
    [(case's line, message)])"""
    ran, bad = 0, []
    for it in range(first, first + count):
        case = make_case(seed, it, trim)
        if case is None:
            continue
        exp = expected(case)
        if verbose:
            out(case.describe())
        ran += 1
        try:
            check(case, exp)
        except AssertionError as e:
            bad.append((case.describe(), str(e)[:400]))
            out("MISMATCH %s: %s" % bad[-1])
    return ran, bad
