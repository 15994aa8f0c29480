"""Crafted pileups for the stages after the pileup (tests only; shared by tests/test_caller_ref_cpu.py and
tests/test_gpu_calls_crafted.py).  Natural pileups -- simulated reads at depth 10^2..10^3 -- never reach what is delicate in
get_baseline_noise and call_variants: two different frequencies within 1e-12 of each other need depths of 10^6, a table that
drains needs hundreds of positions without a minor allele, the filters' thresholds are hit by luck only.  Here every such
situation is a named case; random_mix() draws 200 more from the same building blocks.

A case is a Layout (genome files of random sequences -- nothing is taken from a real genome --, the target file and its cells), the
four u64 arrays in (file, sequence, position, base) order, the call parameters and a name.  No case has more than 10 000 cells.
Everything is seeded through random.Random (Mersenne Twister: the same draws on every Python).
"""
import random

import numpy as np

K = 21
DEFAULTS = dict(k=K, min_af=0.03, no_end_filter=0, no_strand_filter=0, no_strand_balance_filter=0, strand_balance_ratio=0.1,
                n_per_strand=2, strand_odds_max=6.0, min_depth=300, min_variant_depth=3, variant_multiplier=1.5)   # consts.rs:2-21
# every frequency is reported unless the noise bound says no, and that bound is about Noise.max itself (0.5 + 0.5 * 0.03^(100 af)):
# whether the largest values of a window are reported then depends on what the walk and the strip made of it
LOOSE = dict(min_af=1e-9, min_depth=1, min_variant_depth=1, n_per_strand=1, variant_multiplier=0.5)
MARGIN = 1e-9          # a decision through ln() / pow() closer than this to its threshold is not a fair test of anything

_CODE = {65: 0, 67: 1, 71: 2, 84: 3}       # nt_to_bits (lcb.rs:47-55): anything else is 0


class Params:
    """The call parameters of a case; apply() copies them onto any of the three ctypes structures."""

    def __init__(self, **over):
        self.__dict__.update(DEFAULTS)
        self.__dict__.update(over)

    def apply(self, struct):
        for name, v in self.__dict__.items():
            setattr(struct, name, v)
        return struct


def random_sequence(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


class Layout:
    """Genome files [(file name, [(sequence name, bytes)])] and which of them the crafted pileup is for."""

    def __init__(self, name, files, target):
        self.name, self.files, self.target = name, files, target
        self.file_seqs, cell = [], 0
        for _, seqs in files:
            cur = []
            for _, s in seqs:
                cur.append((cell, len(s)))
                cell += len(s)
            self.file_seqs.append(cur)
        self.total_cells = cell
        assert cell <= 10000
        self.seqs = self.file_seqs[target]                                   # [(first cell, length)] of the target
        self.ref_codes = np.array([_CODE.get(c, 0) for _, seqs in files for _, s in seqs for c in s], np.uint8)

    def selection_reads(self):
        """~200 error-free reads of the target's longest sequence: only so that the statistics select the target."""
        seq = max((s for _, s in self.files[self.target][1]), key=len)
        span = min(100, len(seq))
        starts = list(range(0, len(seq) - span + 1, max(1, (len(seq) - span) // 50 or 1)))
        reads = [seq[a:a + span] for a in starts]
        return (reads * (200 // len(reads) + 1))[:max(200, len(reads))]


def _layout(name, seed, decoy_len, lens, edits=()):
    rng = random.Random(seed)
    tgt = [bytearray(random_sequence(rng, n)) for n in lens]
    for s, i, letter in edits:
        tgt[s][i] = ord(letter)
    files = [("decoy", [("d1", random_sequence(rng, decoy_len))]),
             (name, [("%s_s%d" % (name, j), bytes(t)) for j, t in enumerate(tgt)])]
    return Layout(name, files, 1)                      # the target is the second file: its first cell is not cell 0


LENGTHS = [1, 14, 41, 42, 43, 49, 50, 51, 63, 64, 65, 78, 99, 100, 101, 142, 974, 975, 1100]
_layouts = {}


def layout(name):
    if name not in _layouts:
        if name == "lengths":          # len + 50 on both sides of multiples of 64 and 1024; 2k - 1, 2k, 2k + 1; the second of two files
            lay = _layout(name, 11, 150, LENGTHS)
        elif name == "one700":
            lay = _layout(name, 12, 120, [700])
        elif name == "multi":
            lay = _layout(name, 13, 130, [330, 57, 260, 401])
        elif name == "filters":        # the reference letters the filter case wants at its slots
            lay = _layout(name, 14, 150, FILTER_LENS, edits=[(0, 140 + 105 * j, "ACGTN"[j]) for j in range(5)])
        elif name == "tie":            # two genome files with the same sequences: the statistics tie, the lowest id wins
            rng = random.Random(15)
            seqs = [random_sequence(rng, 300), random_sequence(rng, 150)]
            lay = Layout(name, [("twin_a", [("a%d" % j, s) for j, s in enumerate(seqs)]),
                                ("twin_b", [("b%d" % j, s) for j, s in enumerate(seqs)])], 0)
        else:
            raise KeyError(name)
        _layouts[name] = lay
    return _layouts[name]


class Case:
    def __init__(self, name, family, lay, params=None):
        self.name, self.family, self.layout = name, family, lay
        self.params = params or Params()
        n = lay.total_cells * 4
        self.fwd, self.rev, self.fwd_nk, self.rev_nk = (np.zeros(n, np.uint64) for _ in range(4))
        self.nudges = 0

    def arrays(self):
        return self.fwd, self.rev, self.fwd_nk, self.rev_nk

    def with_params(self, name, **over):
        c = Case(name, self.family, self.layout, Params(**dict(self.params.__dict__, **over)))
        c.fwd, c.rev, c.fwd_nk, c.rev_nk = self.fwd, self.rev, self.fwd_nk, self.rev_nk
        return c

    # ---- writing positions ----------------------------------------------------------------------------------------------------
    def put(self, s, i, depth, minors=(), nk=(2, 2), file_seqs=None):
        """Position i of target sequence s: `depth` reads in all, of which minors[j] on the j-th base that is not the reference
        (ascending); every count is split between the strands (forward gets the odd one), every base seen gets nk k-mers."""
        cell0, length = (file_seqs or self.layout.seqs)[s]
        assert 0 <= i < length
        cell = cell0 + i
        ref = int(self.layout.ref_codes[cell])
        others = [b for b in range(4) if b != ref]
        counts = {ref: depth - sum(minors)}
        assert counts[ref] >= 0
        for j, m in enumerate(minors):
            counts[others[j]] = m
        for b in range(4):
            c = counts.get(b, 0)
            self.fwd[cell * 4 + b], self.rev[cell * 4 + b] = c - c // 2, c // 2
            self.fwd_nk[cell * 4 + b], self.rev_nk[cell * 4 + b] = (nk if c else (0, 0))

    def put_strands(self, s, i, ref_fr, alts):
        """Position i of target sequence s with every strand given: ref_fr = (forward, reverse) reads of the reference base, alts =
        [(j, forward, reverse, forward k-mers, reverse k-mers)] for the j-th base that is not the reference."""
        cell0, length = self.layout.seqs[s]
        assert 0 <= i < length
        cell = cell0 + i
        ref = int(self.layout.ref_codes[cell])
        others = [b for b in range(4) if b != ref]
        for b in range(4):
            self.fwd[cell * 4 + b] = self.rev[cell * 4 + b] = self.fwd_nk[cell * 4 + b] = self.rev_nk[cell * 4 + b] = 0
        self.fwd[cell * 4 + ref], self.rev[cell * 4 + ref] = ref_fr
        self.fwd_nk[cell * 4 + ref] = self.rev_nk[cell * 4 + ref] = 2
        for j, f, r, fk, rk in alts:
            b = others[j]
            self.fwd[cell * 4 + b], self.rev[cell * 4 + b], self.fwd_nk[cell * 4 + b], self.rev_nk[cell * 4 + b] = f, r, fk, rk

    def fill(self, s, depth, lo=0, hi=None):
        """coverage without a minor allele"""
        for i in range(lo, self.layout.seqs[s][1] if hi is None else hi):
            self.put(s, i, depth)


# ---- the margins of the decisions that go through ln() and pow() ---------------------------------------------------------------
def reference(case):
    """(records, summary, [(max, mean, std) per sequence], margins) of the case by the Python reference (tests/caller_ref.py), kept
    with the case; margins: [(seq_id, pos, alt, sor margin or None, af margin or None)]"""
    from tests import caller_ref
    if getattr(case, "_ref", None) is None:
        marg, noise = [], []
        recs, summ = caller_ref.call_variants(case.layout.seqs, case.layout.ref_codes, case.fwd, case.rev, case.fwd_nk, case.rev_nk,
                                              case.params, margins=marg, noise=noise)
        case._ref = (recs, summ, noise, marg)
    return case._ref


def too_close(case):
    return [m for m in reference(case)[3] if (m[3] is not None and m[3] < MARGIN) or (m[4] is not None and m[4] < MARGIN)]


def settle(case, max_nudges=3):
    """Move a case away from the thresholds: one more forward read of the reference base at every position that is too close.
    Returns False when that did not help (the caller draws again)."""
    for _ in range(max_nudges):
        bad = too_close(case)
        if not bad:
            return True
        for seq_id, pos, _, _, _ in bad:
            cell = case.layout.seqs[seq_id][0] + pos - 1
            case.fwd[cell * 4 + int(case.layout.ref_codes[cell])] += np.uint64(1)
            case.nudges += 1
        case._ref = None
    return not too_close(case)


# ---- the families ------------------------------------------------------------------------------------------------------------------
def lengths_cases():
    """Every length at which the walk changes shape, every sequence busy: a minor allele at every position (frequencies from a
    handful of values, so that ties and evictions happen), a few calls in each sequence that is long enough."""
    lay = layout("lengths")
    c = Case("lengths", "lengths", lay, Params(**LOOSE))
    rng = random.Random(101)
    for s, (_, length) in enumerate(lay.seqs):
        for i in range(length):
            c.put(s, i, 1000, [rng.choice([1, 2, 3, 5, 8, 13, 40])] + ([rng.choice([1, 2])] if rng.random() < 0.3 else []))
    return [c, c.with_params("lengths_no_end", no_end_filter=1), c.with_params("lengths_default", **DEFAULTS)]


def near_tie_cases():
    lay = layout("one700")
    out = []
    # minor counts of 1 at depths 999 999 / 1 000 000 / 1 000 001: 1/999999 - 1/1000000 > 1e-12 > 1/1000000 - 1/1000001.  All six
    # orders of the three along the sequence, a window apart; every other position has no minor allele: these values are the table
    c = Case("near_ties_count1", "near_ties", lay, Params(**LOOSE))
    c.fill(0, 1000)
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for g, perm in enumerate(perms):
        for j, d in enumerate(perm):
            c.put(0, 10 + 110 * g + 3 * j, 999999 + d, [1])
    out.append(c)
    # counts of 2 at depths 1 414 212 .. 1 414 216: neighbours 1e-12 apart (either side of it), next-but-one neighbours 2e-12 apart
    c = Case("near_ties_count2", "near_ties", lay, Params(**LOOSE))
    c.fill(0, 1000)
    orders = [(0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 0, 4, 1, 3), (1, 3, 0, 4, 2), (3, 4, 0, 1, 2), (0, 2, 4, 3, 1)]
    for g, order in enumerate(orders):
        for j, d in enumerate(order):
            c.put(0, 5 + 110 * g + 4 * j, 1414212 + d, [2])
    out.append(c)
    # a full table and an eleventh value v just below its smallest entry t.  v comes first, so it falls off the table when the
    # eleventh value arrives, and leaves first; t comes last and leaves last:
    #   group 0  t - v < 1e-12 (count 1): leaving, v evicts t -- an entry that is not its own; t then sits in the window without an entry
    #   group 1  the same with counts of 2
    #   group 2  t - v in (1e-12, 2e-12]: takes the exact test, evicts nothing
    #   group 3  t - v > 2e-12: passed by
    c = Case("near_ties_eleventh", "near_ties", lay, Params(**LOOSE))
    c.fill(0, 1000)
    pairs = [((1, 1000001), (1, 1000000)), ((2, 1414215), (2, 1414214)), ((2, 1414215), (2, 1414213)), ((2, 1414213), (2, 1414211))]
    for g, (v, t) in enumerate(pairs):
        for j, (cnt, d) in enumerate([v] + [(3 + q, 1000000) for q in range(9)] + [t]):
            c.put(0, 4 + 170 * g + 2 * j, d, [cnt])
    out.append(c)
    # ten values, then v, which is never inserted (the table is full of larger ones), then -- once the table has room again -- t within
    # 1e-12 of v: leaving, v evicts t although v never was in the table.  The same with t in the band, where nothing happens.
    c = Case("near_ties_never_inserted", "near_ties", lay, Params(**LOOSE))
    c.fill(0, 1000)
    for g, (v, t) in enumerate(pairs[:3]):
        base = 3 + 230 * g
        for q in range(10):
            c.put(0, base + 2 * q, 1000000, [3 + q])
        c.put(0, base + 20, v[1], [v[0]])
        c.put(0, base + 103, t[1], [t[0]])
    out.append(c)
    return out


def exact_tie_cases():
    lay = layout("one700")
    # (a multiplier of 0.7: with 0.5 an allele at half the noise level -- 1/10 under 1/5 -- would sit exactly on the bound)
    c = Case("exact_ties", "exact_ties", lay, Params(**dict(LOOSE, variant_multiplier=0.7)))
    c.fill(0, 900)
    thirds = [(3, 1), (6, 2), (15, 5), (300, 100), (999, 333)]
    for j in range(15):                                  # more than ten equal values in a window: 1/3 from five different counts
        d, m = thirds[j % 5]
        c.put(0, 10 + j, d, [m])
    dup = [(15, 3), (5, 1), (10, 2), (10, 1), (20, 2), (30, 3), (20, 1), (25, 1), (40, 2), (100, 5), (50, 1), (50, 1)]
    for j, (d, m) in enumerate(dup):                     # duplicates inside the table: 1/5 three times, 1/10 three times, 1/20 ...
        c.put(0, 200 + 3 * j, d, [m])
    for j in range(12):                                  # twelve times 1/1000 and three larger values among them
        c.put(0, 400 + 2 * j, 1000 * (1 + j % 3), [1 + j % 3])
    for j, m in enumerate([7, 9, 7]):
        c.put(0, 401 + 6 * j, 1000, [m])
    for j in range(30):                                  # equal values on three ranks at once
        c.put(0, 560 + j, 1200, [100, 100, 100] if j % 2 else [100, 100])
    return [c]


def table_life_cases():
    out = []
    rng = random.Random(301)
    lay = layout("multi")
    c = Case("table_full", "table_life", lay, Params(**LOOSE))
    for s, (_, length) in enumerate(lay.seqs):
        for i in range(length):
            c.put(s, i, 5000, [rng.randrange(1, 400)])
    out.append(c)
    # coverage with minor alleles, >= 100 positions with no coverage, >= 100 with coverage and no minor allele, minor alleles again
    c = Case("table_drain_refill", "table_life", layout("one700"), Params(**LOOSE))
    for i in range(700):
        if i < 150 or i >= 390:
            c.put(0, i, 2000, [rng.randrange(1, 300)])
        elif i >= 270:
            c.put(0, i, 2000)
    out.append(c)
    c = Case("table_never_fills", "table_life", layout("one700"), Params(**LOOSE))
    c.fill(0, 800)
    for i in range(3, 700, 15):
        c.put(0, i, 800, [rng.randrange(1, 100)])
    out.append(c)
    # strictly increasing / decreasing at every position of every sequence: every step changes the table, the list of its states runs
    # to len + 51 of the len + 64 a sequence is allowed
    for name, sign in (("table_increasing", 1), ("table_decreasing", -1)):
        lay = layout("lengths")
        c = Case(name, "table_life", lay, Params(**LOOSE))
        for s, (_, length) in enumerate(lay.seqs):
            for i in range(length):
                c.put(s, i, 10000, [i + 1 if sign > 0 else length - i])
        out.append(c)
    return out


def three_rank_cases():
    lay = layout("one700")
    c = Case("three_ranks", "three_ranks", lay, Params(**LOOSE))
    rng = random.Random(401)
    c.fill(0, 3000)
    for i in range(7, 700, 9):
        c.put(0, i, 3000, [rng.randrange(1, 30)])
    for j, i in enumerate(range(20, 700, 100)):          # 100 apart: one step evicts three values and inserts three
        c.put(0, i, 3000, [300 + 10 * j, 200 + j, 90 - j])
    return [c]


def strip_cases():
    lay = layout("one700")
    out = []
    c = Case("strip_n_1_2_3", "strip", lay, Params(**LOOSE))
    c.fill(0, 1000)
    c.put(0, 50, 1000, [40])                             # alone: n = 1, tau = inf
    c.put(0, 250, 1000, [40]); c.put(0, 280, 1000, [7])                                   # noqa: E702 -- n = 1, 2, 1
    c.put(0, 450, 1000, [400]); c.put(0, 470, 1000, [3]); c.put(0, 490, 1000, [2])        # noqa: E702 -- n up to 3: the first finite tau
    c.put(0, 650, 1000, [5, 5, 5])                       # n = 3 of one value: var = 0
    out.append(c)
    c = Case("strip_identical", "strip", lay, Params(**LOOSE))
    c.fill(0, 1000)
    for i in range(10, 70):
        c.put(0, i, 1000, [1])                           # var = 0 or a rounding residue of either sign
    for i in range(200, 290):
        c.put(0, i, 3, [1])                              # 1/3 is not exact
    for i in range(420, 560):
        c.put(0, i, 1000, [7])
    out.append(c)
    c = Case("strip_outlier", "strip", lay, Params(**LOOSE))
    rng = random.Random(501)
    for i in range(700):
        c.put(0, i, 100000, [rng.randrange(1, 4)])
    for i in (60, 300, 330, 600):
        c.put(0, i, 1000, [400])                         # after it is stripped, `curr_s2 -= candidate` leaves a negative variance
    out.append(c)
    c = Case("strip_n_300", "strip", lay, Params(**LOOSE))
    c.fill(0, 1000)
    for i in range(100, 320):
        c.put(0, i, 1000, [10, 10, 10])                  # 300 equal values: the last entry of the Student-t table
    for i in range(420, 600):
        c.put(0, i, 1000, [10 + i % 3, 10, 9])
    out.append(c)
    # as many entries stripped as a pileup allows.  Every strip takes the candidate, not its square, off the sum of squares (the quirk
    # of call.rs:936), so the variance turns negative -- NaN, nothing is an outlier -- after a few: with frequencies of at most 1/2
    # a grid search over windows found none in which more than seven of the ten go.  This is that window (ten positions at 1/2,
    # 86 at 106/1000 with two alleles at 1/1000, four at 1/1000 three times), repeated along the sequence.
    c = Case("strip_seven", "strip", lay, Params(**LOOSE))
    c.fill(0, 1000)
    for i in range(100, 600):
        c.put(0, i, 1000, [500] if i % 10 == 0 else [1, 1, 1] if i % 25 == 1 else [106, 1, 1])
    out.append(c)
    return out


FILTER_LENS = [2900, 2000, 45, 43, 42, 41, 14]


def filter_cases():
    """Every filter of call_variants at its threshold.  The background is a minor allele of 1..3 reads in 5000 at every position: an
    edit is then an outlier of its window, it is stripped, and Noise.max is the background's -- the edits sit more than a window
    apart (in one window the second largest edit would be the noise level of the largest)."""
    lay = layout("filters")
    c = Case("filters_default", "filters", lay)
    rng = random.Random(601)
    for s, (_, length) in enumerate(lay.seqs):
        for i in range(length):
            c.put(s, i, 5000, [rng.randrange(1, 4)])
    slot = lambda j: 140 + 105 * j                                                         # noqa: E731
    edits = [
        ((450, 450), [(0, 50, 50, 2, 2)]),                # 0..4: the reference base is A, C, G, T and N (an N counts as A)
        ((450, 450), [(1, 50, 50, 2, 2)]),
        ((450, 450), [(2, 50, 50, 2, 2)]),
        ((450, 450), [(0, 50, 50, 2, 2)]),
        ((450, 450), [(1, 50, 50, 2, 2)]),
        ((145, 145), [(0, 10, 0, 2, 0)]),                 # 5: the alternative on the forward strand only, SOR below the limit
        ((450, 450), [(2, 100, 0, 2, 0)]),                # 6: ... and above it
        ((450, 450), [(1, 0, 100, 0, 2)]),                # 7: on the reverse strand only
        ((485, 485), [(0, 15, 15, 2, 2)]),                # 8: af = 30/1000 = min_af exactly: reported
        ((146, 145), [(0, 5, 4, 2, 2)]),                  # 9: af = 9/300 = min_af exactly at depth = min_depth
        ((486, 485), [(0, 15, 14, 2, 2)]),                # 10: af = 29/1000: not reported
        ((50, 50), [(0, 50, 50, 2, 2)]),                  # 11: af = 1/2 exactly: a major variant, whatever the depth
        ((75, 75), [(1, 75, 74, 2, 2)]),                  # 12: af = 149/299, depth 299: a minor variant below min_depth
        ((76, 75), [(1, 75, 74, 2, 2)]),                  # 13: af = 149/300, depth 300: reported
        ((135, 134), [(2, 15, 15, 2, 2)]),                # 14: depth 299, af = 30/299
        ((135, 135), [(2, 15, 15, 2, 2)]),                # 15: depth 300
        ((450, 450), [(0, 50, 50, 1, 1)]),                # 16..19: k-mer support 1 / 2 on either strand
        ((450, 450), [(0, 50, 50, 1, 2)]),
        ((450, 450), [(0, 50, 50, 2, 1)]),
        ((450, 450), [(0, 50, 50, 2, 2)]),
        ((5, 895), [(1, 0, 100, 0, 2)]),                  # 20: nearly everything on one strand: sor = -1 when the balance filter is off
        ((200, 200), [(0, 100, 100, 2, 2), (1, 100, 100, 2, 2), (2, 100, 100, 2, 2)]),   # 21: all three alternatives pass
        ((1 << 40, (1 << 40) - 5), [(0, 1 << 38, (1 << 38) + 3, 2, 2)]),                # 22: counts up to 2^40
        ((499, 499), [(0, 1, 1, 2, 2)]),                  # 23: alternative depth 2 (af 2/1000: filters_loose)
        ((499, 498), [(0, 2, 1, 2, 2)]),                  # 24: alternative depth 3
    ]
    assert slot(len(edits) - 1) < FILTER_LENS[0] - K - 100
    for j, (ref_fr, alts) in enumerate(edits):
        c.put_strands(0, slot(j), ref_fr, alts)
    edit = ((450, 450), [(0, 50, 50, 2, 2)])
    c.put_strands(0, K, *edit)                            # positions k and len - k of one sequence, k - 1 and len - k - 1 of another
    c.put_strands(0, FILTER_LENS[0] - K, *edit)
    c.put_strands(1, K - 1, *edit)
    c.put_strands(1, FILTER_LENS[1] - K - 1, *edit)
    c.put_strands(2, 45 - K - 1, *edit)                   # len = 2k + 3: positions 21..23 are inside
    c.put_strands(3, K, *edit)                            # len = 2k + 1: position 21 alone
    c.put_strands(4, K, *edit)                            # len = 2k: nothing is inside
    c.put_strands(5, K - 1, *edit)                        # len = 2k - 1
    c.put_strands(6, 7, *edit)                            # len < k
    return [c,
            c.with_params("filters_no_end", no_end_filter=1),
            c.with_params("filters_no_strand", no_strand_filter=1),
            c.with_params("filters_no_balance", no_strand_balance_filter=1),
            c.with_params("filters_no_balance_03", no_strand_balance_filter=1, strand_balance_ratio=0.3),
            c.with_params("filters_loose", min_af=0.001, n_per_strand=1, strand_odds_max=10.0, variant_multiplier=0.3),
            c.with_params("filters_strict", min_variant_depth=31, min_depth=301, n_per_strand=3)]


def tie_case():
    """The selection tie: the pileup of twin_a (file 0); twin_b's cells hold other numbers, which a wrong choice would read."""
    lay = layout("tie")
    c = Case("selection_tie", "selection", lay, Params(**LOOSE))
    rng = random.Random(701)
    for s, (_, length) in enumerate(lay.seqs):
        for i in range(length):
            c.put(s, i, 2000, [rng.randrange(1, 200)])
            c.put(s, i, 700, [rng.randrange(1, 300)], file_seqs=lay.file_seqs[1])
    return c


def sparse_lengths_case():
    """A few values per sequence on the layout of table_increasing: run after it on one engine, it reads the same state lists."""
    lay = layout("lengths")
    c = Case("lengths_sparse", "table_life", lay, Params(**LOOSE))
    rng = random.Random(801)
    for s, (_, length) in enumerate(lay.seqs):
        c.fill(s, 4000)
        for i in range(s % 7, length, 37):
            c.put(s, i, 4000, [rng.randrange(1, 90)])
    return c


def named_cases():
    return (lengths_cases() + near_tie_cases() + exact_tie_cases() + table_life_cases() + three_rank_cases() + strip_cases() +
            filter_cases() + [sparse_lengths_case(), tie_case()])


# ---- the random mix -------------------------------------------------------------------------------------------------------------
_NEAR = [(1, 999999), (1, 1000000), (1, 1000001), (2, 1414212), (2, 1414213), (2, 1414214), (2, 1414215), (2, 1414216)]
_TIES = [(3, 1), (6, 2), (15, 5), (10, 1), (20, 2), (1000, 1), (3000, 3), (5, 1), (25, 5)]
_PARAMS = [dict(), dict(LOOSE), dict(no_end_filter=1, min_af=0.01), dict(no_strand_filter=1, min_depth=10),
           dict(no_strand_balance_filter=1, strand_balance_ratio=0.3, min_af=0.001), dict(LOOSE, variant_multiplier=0.5),
           dict(min_af=0.005, min_depth=10, min_variant_depth=1, n_per_strand=1, variant_multiplier=2.0, strand_odds_max=8.0)]


def _random_segment(c, rng, s, lo, hi):
    kind = rng.choice(["none", "clean", "bulk", "bulk", "ties", "near", "up", "down", "three", "sparse"])
    depth = rng.choice([299, 300, 1000, 5000, 100000])
    for i in range(lo, hi):
        if kind == "none":
            continue
        if kind == "clean":
            c.put(s, i, depth)
        elif kind == "bulk":
            c.put(s, i, 5000, [rng.randrange(1, 6)], nk=(rng.randrange(1, 4), rng.randrange(1, 4)))
        elif kind == "ties":
            d, m = rng.choice(_TIES)
            c.put(s, i, d, [m])
        elif kind == "near":
            m, d = rng.choice(_NEAR)
            c.put(s, i, d, [m] if rng.random() < 0.5 else [])
        elif kind == "up":
            c.put(s, i, 20000, [1 + (i - lo) * 3])
        elif kind == "down":
            c.put(s, i, 20000, [1 + (hi - i) * 3])
        elif kind == "three":
            c.put(s, i, 2000, [rng.randrange(1, 100), rng.randrange(1, 50), rng.randrange(1, 20)] if rng.random() < 0.4 else [])
        else:
            c.put(s, i, depth, [rng.randrange(1, 30)] if rng.random() < 0.08 else [])
    for _ in range(rng.randrange(0, 3)):                 # edits: any strands, any k-mer support
        i = rng.randrange(lo, hi)
        d = rng.choice([299, 300, 1000])
        alt = rng.randrange(1, d // 2 + 1)
        af = rng.randrange(0, alt + 1)
        rf = rng.randrange(0, d - alt + 1)
        c.put_strands(s, i, (rf, d - alt - rf), [(rng.randrange(3), af, alt - af, rng.randrange(0, 4), rng.randrange(0, 4))])


def random_case(n, attempt=0):
    rng = random.Random(100000 + 1000 * attempt + n)
    lay = layout("lengths" if n % 25 == 24 else rng.choice(["multi", "multi", "one700"]))
    c = Case("random_%03d" % n if not attempt else "random_%03d_redraw%d" % (n, attempt), "random", lay, Params(**rng.choice(_PARAMS)))
    for s, (_, length) in enumerate(lay.seqs):
        lo = 0
        while lo < length:
            hi = min(length, lo + rng.randrange(20, 180))
            _random_segment(c, rng, s, lo, hi)
            lo = hi
    return c


def random_mix(count=200):
    """(cases, number of pileups that had to be drawn again because a decision stayed within MARGIN of its threshold)"""
    out, redrawn = [], 0
    for n in range(count):
        attempt = 0
        c = random_case(n)
        while not settle(c):
            attempt += 1
            c = random_case(n, attempt)
        redrawn += 1 if attempt else 0
        out.append(c)
    return out, redrawn
