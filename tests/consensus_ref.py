"""The consensus rule of `bronko call --consensus` restated in plain Python, and the crafted pileups it is tested on (tests only;
shared by tests/test_consensus_cpu.py and tests/test_gpu_consensus.py).  Written from the rule's definition (include/bronko_hip.h,
bk_sample_consensus), not from the C++ or the kernel: Python ints, sorted(), and one float product.

    tot[b] = forward + reverse depth of base b (A C G T), depth = their sum
    depth < D                      N, masked
    else                           the bases by descending tot (equal counts: ascending code) are taken, their counts summed in cum,
                                   until float(cum) >= F * float(depth); then every further base whose count equals the last taken
                                   one's; a count of 0 is never taken; the set as a bit mask indexes "-ACMGRSVTWYHKDBN"
    one base: called (a substitution if it is not the reference code of the cell); more: ambiguous
"""
import functools
import itertools
import random

from tests import pileup_cases

LETTERS = "-ACMGRSVTWYHKDBN"               # by bit mask A = 1, C = 2, G = 4, T = 8
PARAMS = [(1, 0.0), (10, 0.5), (300, 0.75), (1, 1.0)]   # (D, F) every pileup is checked at
TALLIES = ("positions", "called", "ambiguous", "masked", "substitutions")


@functools.lru_cache(maxsize=None)
def base_set(tot, min_depth, min_freq):
    """The bit mask of the bases taken at a position with the four counts `tot`; None when the position is masked."""
    depth = sum(tot)
    if depth < min_depth:
        return None
    order = sorted(range(4), key=lambda b: (-tot[b], b))
    taken, cum = [], 0
    for b in order:
        if tot[b] == 0:
            break
        taken.append(b)
        cum += tot[b]
        if float(cum) >= min_freq * float(depth):
            break
    for b in order[len(taken):]:
        if tot[b] != 0 and tot[b] == tot[taken[-1]]:
            taken.append(b)
    mask = 0
    for b in taken:
        mask |= 1 << b
    return mask


def consensus(seqs, ref_codes, fwd, rev, min_depth, min_freq):
    """(letters as bytes, {tally: count}) of the sequences [(first cell, length)] of one genome on the two depth arrays of all cells."""
    fwd, rev, ref_codes = fwd.tolist(), rev.tolist(), ref_codes.tolist()
    letters = bytearray()
    t = dict.fromkeys(TALLIES, 0)
    for cell0, length in seqs:
        for cell in range(cell0, cell0 + length):
            tot = tuple(fwd[cell * 4 + b] + rev[cell * 4 + b] for b in range(4))
            mask = base_set(tot, min_depth, min_freq)
            t["positions"] += 1
            if mask is None:
                letters.append(ord("N"))
                t["masked"] += 1
                continue
            letters.append(ord(LETTERS[mask]))
            if mask & (mask - 1) == 0:
                t["called"] += 1
                if mask != 1 << ref_codes[cell]:
                    t["substitutions"] += 1
            else:
                t["ambiguous"] += 1
    return bytes(letters), t


def fasta_text(stem, names, seqs, letters):
    """What write_consensus_fasta writes: a record per sequence, ">stem|name", lines of 60."""
    out, at = [], 0
    for name, (_, length) in zip(names, seqs):
        out.append(">%s|%s\n" % (stem, name))
        for i in range(0, length, 60):
            out.append(letters[at + i:at + min(i + 60, length)].decode() + "\n")
        at += length
    return "".join(out).encode()


def params_of(case):
    """The (D, F) pairs a case is checked at: the four of every pileup and what the case itself asks for."""
    return PARAMS + list(getattr(case, "extra_params", ()))


def expected(case, min_depth, min_freq):
    """consensus() of the case's target genome, computed once and kept with the case."""
    kept = case.__dict__.setdefault("_consensus_ref", {})
    if (min_depth, min_freq) not in kept:
        lay = case.layout
        kept[(min_depth, min_freq)] = consensus(lay.seqs, lay.ref_codes, case.fwd, case.rev, min_depth, min_freq)
    return kept[(min_depth, min_freq)]


# ---- the crafted pileups ------------------------------------------------------------------------------------------------------------
def put_counts(case, s, i, counts, strand="both"):
    """Position i of target sequence s with `counts` reads of A, C, G, T: split between the strands (forward gets the odd one), all on the
    forward or all on the reverse strand, or -- "each" -- that many on either strand."""
    def fr(c):
        return {"both": (c - c // 2, c // 2), "fwd": (c, 0), "rev": (0, c), "each": (c, c)}[strand]
    cell0, _ = case.layout.seqs[s]
    ref = int(case.layout.ref_codes[cell0 + i])
    others = [b for b in range(4) if b != ref]
    case.put_strands(s, i, fr(counts[ref]), [(j,) + fr(counts[b]) + (2, 2) for j, b in enumerate(others)])


def _all_on(ref, depth, shift=0):
    c = [0, 0, 0, 0]
    c[(ref + shift) % 4] = depth
    return c


@functools.lru_cache(maxsize=None)
def crafted_cases():
    Case, layout = pileup_cases.Case, pileup_cases.layout
    out = []

    # every length: each position of each sequence but one takes one of a handful of patterns (relative to its reference base); the decoy
    # genome in front of the target is covered deeply with bases that are not its reference -- nothing of it may show
    lay = layout("lengths")
    c = Case("consensus_lengths", "consensus", lay)
    rng = random.Random(901)
    patterns = [(40, 0, 0, 0), (9, 0, 0, 0), (0, 25, 0, 0), (30, 30, 0, 0), (50, 30, 20, 0), (5, 5, 5, 5), (0, 0, 0, 0), (301, 100, 0, 0),
                (0, 7, 3, 0), (1, 0, 0, 0)]
    for s, (cell0, length) in enumerate(lay.seqs):
        if s == 7:
            continue                                      # a sequence with no coverage at all
        for i in range(length):
            ref = int(lay.ref_codes[cell0 + i])
            p = rng.choice(patterns)
            put_counts(c, s, i, [p[(b - ref) % 4] for b in range(4)])
    for i in range(lay.file_seqs[0][0][1]):
        c.put(0, i, 90000, [60000, 20000, 10000], file_seqs=lay.file_seqs[0])
    out.append(c)

    # the same files with the short genome in front as the target: on one engine after consensus_lengths, its 150 letters and its
    # tallies are all there may be
    short = pileup_cases.Layout("lengths", lay.files, 0)
    c = Case("consensus_short_genome", "consensus", short)
    for i in range(short.seqs[0][1]):
        ref = int(short.ref_codes[i])
        p = patterns[i % len(patterns)]
        put_counts(c, 0, i, [p[(b - ref) % 4] for b in range(4)])
    out.append(c)

    # the rule, position by position, on the four sequences of "multi" (the third stays without coverage)
    lay = layout("multi")
    c = Case("consensus_rule", "consensus", lay)
    c.extra_params = [(1, 1.0 / 3.0), (1, 0.7), (10, 1.0 / 3.0), (300, 0.5)]
    at = iter(range(lay.seqs[0][1]))
    for perm in itertools.permutations((40, 30, 20, 10)):        # all 24 orderings of four distinct counts
        put_counts(c, 0, next(at), list(perm))
    for mask in range(1, 16):                                    # each of the 15 base sets: equal counts on its bases
        put_counts(c, 0, next(at), [20 if mask >> b & 1 else 0 for b in range(4)])
    for mask in range(1, 16):                                    # ... and deep enough for D = 300
        put_counts(c, 0, next(at), [400 if mask >> b & 1 else 0 for b in range(4)])
    shares = [(50, 50, 0, 0), (50, 30, 20, 0), (49, 31, 20, 0), (40, 30, 30, 0), (25, 25, 25, 25),   # 50/50: equality stops the walk, the tie adds the second
              (30, 30, 10, 0), (30, 10, 5, 0),                   # F = 0: the top base only, and a tie at the top
              (5, 3, 1, 0), (6, 0, 0, 1),                        # F = 1: every base that was seen
              (1, 1, 1, 0), (2, 1, 0, 0), (1, 2, 0, 0), (3, 0, 0, 0),                # depth 3 at F = 1/3 and 0.7
              (3, 2, 2, 0), (4, 3, 0, 0), (2, 2, 2, 1), (1, 2, 4, 0), (5, 1, 1, 0), (3, 3, 1, 0), (7, 0, 0, 0),   # depth 7
              (150, 100, 50, 0), (225, 75, 0, 0), (224, 76, 0, 0), (100, 100, 100, 0)]   # depth 300 at F = 0.75
    for p in shares:
        for rot in range(4):                                     # every pattern on every base
            put_counts(c, 0, next(at), [p[(b - rot) % 4] for b in range(4)])
    ref_at = lambda s, i: int(lay.ref_codes[lay.seqs[s][0] + i])                         # noqa: E731
    i = 0
    for d in (0, 1, 2, 9, 10, 11, 299, 300, 301):               # depth D - 1, D, D + 1: on the reference base, on another one, on two
        put_counts(c, 1, i, _all_on(ref_at(1, i), d)); i += 1                            # noqa: E702
        put_counts(c, 1, i, _all_on(ref_at(1, i), d, shift=1)); i += 1                   # noqa: E702
        put_counts(c, 1, i, [d - d // 2, d // 2, 0, 0]); i += 1                          # noqa: E702
    i = 0
    for strand in ("fwd", "rev"):                                # counts on one strand only
        for p in ((40, 0, 0, 0), (0, 12, 0, 0), (20, 20, 0, 0), (9, 0, 0, 0), (0, 0, 300, 100)):
            put_counts(c, 3, i, list(p), strand); i += 1                                 # noqa: E702
    big = 10 ** 12
    for p in ((big, 0, 0, 0), (0, big, big - 1, 0), (big, big, 0, 0), (big, big - 1, big - 2, big - 3), (0, 0, big, 1)):   # 10^12 per strand
        put_counts(c, 3, i, list(p), "each"); i += 1                                     # noqa: E702
    out.append(c)

    # "filters": the reference letters A, C, G, T and N at their slots (an N counts as A), each with every base on top in turn
    lay = layout("filters")
    for shift in range(4):
        c = Case("consensus_ref_letters_%d" % shift, "consensus", lay)
        for j in range(5):
            i = 140 + 105 * j
            assert lay.files[1][1][0][1][i:i + 1] == b"ACGTN"[j:j + 1]
            put_counts(c, 0, i, _all_on(int(lay.ref_codes[lay.seqs[0][0] + i]), 50, shift))
            put_counts(c, 0, i + 1, [12, 12, 0, 0])
        c.fill(1, 20, 0, 300)
        put_counts(c, 6, 13, _all_on(int(lay.ref_codes[lay.seqs[6][0] + 13]), 33, shift))   # the last position of the last sequence
        out.append(c)

    # "tie": the twin genome's cells hold other bases, which a wrong selection would read
    lay = layout("tie")
    c = Case("consensus_twin", "consensus", lay)
    rng = random.Random(902)
    for s, (cell0, length) in enumerate(lay.seqs):
        for i in range(length):
            depth = rng.choice([8, 40, 400])
            c.put(s, i, depth, [rng.choice([0, 1, 4, depth // 2])] if rng.random() < 0.5 else [])
            c.put(s, i, 500, [400, 60], file_seqs=lay.file_seqs[1])
    out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_cases():
    return tuple(pileup_cases.random_mix(200)[0])


@functools.lru_cache(maxsize=None)
def named_cases():
    return tuple(pileup_cases.named_cases())


def coverage_of(cases):
    """(the base sets, whether a masked and whether an unmasked position) that occur over the cases at their parameters."""
    sets, masked, unmasked = set(), False, False
    for case in cases:
        lay = case.layout
        fwd, rev = case.fwd.tolist(), case.rev.tolist()
        for d, f in params_of(case):
            for cell0, length in lay.seqs:
                for cell in range(cell0, cell0 + length):
                    m = base_set(tuple(fwd[cell * 4 + b] + rev[cell * 4 + b] for b in range(4)), d, f)
                    if m is None:
                        masked = True
                    else:
                        unmasked = True
                        sets.add(m)
    return sets, masked, unmasked
