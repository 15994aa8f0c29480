"""Inputs of the junction tests (tests/test_junctions_cpu.py, tests/test_gpu_junctions.py): crafted records on the indel tests'
crafted genome, and a sample of random reads of a genome with planted junctions.  What the rule makes of them is junctions_ref's
business."""
from __future__ import annotations

import random

from tests import indel_cases, junctions_ref
from tests.indel_cases import _free_pos, _rand, mut_read

N_LEN = 150


def crafted_genome(k: int):
    """indel_cases.crafted_genome(k) -- craftA with a homopolymer run [300, 312), a dinucleotide repeat [500, 520), a repeat of
    k + 24 bases and a stretch of N [1300, 1320), and craftB -- and behind them craftC: random letters in which three stretches
    occur twice, of exactly 1, 6 and k - 1 bases (the letters around each copy differ, and no shared stretch holds a k-mer).  That
    genome has no pair of stretches that agree in exactly that many bases, and its sequences' cells stay where they are."""
    rng = random.Random(2000 + k)
    c = list(_rand(rng, 1000))
    for (x, y, h) in homology_sites(k).values():
        c[y:y + h] = c[x:x + h]
        for u, v in ((x - 1, y - 1), (x + h, y + h)):   # the shared stretch ends on both sides
            c[v] = "ACGT"[("ACGT".index(c[u]) + 1) % 4]
    return indel_cases.crafted_genome(k) + [("craftC", "".join(c))]


def homology_sites(k: int):
    """label -> (first copy, second copy, length) of craftC's shared stretches, as offsets in craftC"""
    return {"one": (200, 560, 1), "six": (300, 700, 6), "k_minus_1": (400, 830, k - 1)}


def _set(read: str, off: int, base: str) -> str:
    return read[:off] + base + read[off + 1:]


def _other(*bases):
    return next(c for c in "ACGT" if c not in bases)


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(k); every read is there along and against the reference (label + '/rc').
    expect, at min_len 33 and 2 mismatches: ('jn', cell, D) the junction the record supports as planted (before normalisation),
    'span', 'short', 'backward', 'discordant', or 'none' for a record that leaves no tally behind `anchored`."""
    (_, a), (_, b), (_, c) = crafted_genome(k)
    first_b, first_c = len(a), len(a) + len(b)
    text = a + b + c
    n = N_LEN
    cases = []

    def jn(ref, pos, d, start=None, length=n, subs=()):
        return mut_read(ref, pos - 70 if start is None else start, length, dele=(pos, d), subs=subs)

    p33, p400 = _free_pos(a, 800, 33), _free_pos(a, 760, 400)
    cases.append(("d33", jn(a, p33, 33), ("jn", p33, 33)))
    cases.append(("d400", jn(a, p400, 400), ("jn", p400, 400)))
    # as far as craftA lets a record jump: from its start to the last cells in front of the run of N; and across nearly all of craftB
    p_far = _free_pos(a, 75, 1135)
    cases.append(("a_start_to_end", jn(a, p_far, 1135), ("jn", p_far, 1135)))
    pb = _free_pos(b, k + 80, 530)
    cases.append(("b_start_to_end", jn(b, pb, 530), ("jn", first_b + pb, 530)))
    for d in (32, 1):
        pos = _free_pos(a, 800, d)
        cases.append(("d%d" % d, jn(a, pos, d), "short"))
    # the flanks share 1, 6, k - 1 bases: the record breaks in the middle of the shared stretch (at its end for one base)
    for label, (x, y, h) in homology_sites(k).items():
        bp = x + (h + 1) // 2
        cases.append(("homology_" + label, jn(c, bp, y - x), ("jn", first_c + bp, y - x)))
    cases.append(("in_homopolymer", jn(a, 306, 400), ("jn", 306, 400)))
    cases.append(("in_dinucleotide", jn(a, 510, 300), ("jn", 510, 300)))
    cases.append(("m_eq_M", jn(a, p400, 400, subs=(40, 100)), ("jn", p400, 400)))
    cases.append(("m_eq_M_plus_1", jn(a, p400, 400, subs=(40, 60, 100)), "discordant"))
    # the last base in front of the breakpoint reads as the base in front of the acceptor: one to the left fits without a mismatch;
    # the first base behind it reads as the first base left out: one to the right does
    plain = jn(a, p400, 400)
    cases.append(("sub_left_of_bp", _set(plain, 69, a[p400 + 399]), ("jn", p400 - 1, 400)))
    if a[p400] != a[p400 + 400]:
        cases.append(("sub_right_of_bp", _set(plain, 70, a[p400]), ("jn", p400 + 1, 400)))
    # the first base behind the breakpoint fits neither side: p and p + 1 tie at one mismatch, the smaller wins
    cases.append(("tie", _set(plain, 70, _other(a[p400], a[p400 + 400])), ("jn", p400, 400)))
    cases.append(("anchor_try2_front", jn(a, p400, 400, subs=(3,)), ("jn", p400, 400)))
    cases.append(("anchor_try2_back", jn(a, p400, 400, subs=(n - 4,)), ("jn", p400, 400)))
    cases.append(("backward_100", a[900:975] + a[875:950], "backward"))
    cases.append(("a_and_b", a[700:775] + b[100:175], "none"))
    cases.append(("over_N", a[1200:1275] + a[1340:1415], "none"))
    cases.append(("leaves_sequence", a[1330:1405] + a[1440:1500] + b[:15], "none"))
    cases.append(("bp_at_a_plus_k", jn(a, p400, 400, start=p400 - k), ("jn", p400, 400)))
    cases.append(("bp_at_b", jn(a, p400, 400, start=p400 - (n - k)), ("jn", p400, 400)))
    cases.append(("bp_in_last_k", jn(a, p400, 400, start=p400 - (n - k + 5)), None))
    cases.append(("n_2k", jn(a, p400, 400, start=p400 - k, length=2 * k), ("jn", p400, 400)))
    cases.append(("n_2k_minus_1", jn(a, p400, 400, start=p400 - k, length=2 * k - 1), "none"))
    cases.append(("n_300", jn(a, p33, 33, start=p33 - 150, length=300), ("jn", p33, 33)))
    cases.append(("plain_over_donor", a[p400 - 70:p400 + 80], "span"))
    cases.append(("plain_over_acceptor", a[p400 + 330:p400 + 480], "span"))
    cases.append(("plain_mismatches", mut_read(a, 900, n, subs=(40, 60, 100)), "discordant"))
    out = []
    for label, read, expect in cases:
        assert set(read) <= set("ACGT"), label
        out.append((label, read, expect))
        out.append((label + "/rc", junctions_ref.revcomp(read), expect))
    return out, text


def haplotype(text: str, cell: int, d: int) -> str:
    """The genome with one junction applied"""
    return text[:cell] + text[cell + d:]


PLANTED = [(1000, 500, 0.6), (2000, 3000, 0.5), (3500, 40, 0.3), (5200, 33, 0.5)]   # (cell, D, frequency)
SHORT = (4000, 6, 0.5)             # a deletion that --indels reports
SAMPLE_SPAN = (800, 5600)          # the reads start in these cells of the genome
SAMPLE_SEED = 1


def sample_reads(g: str, seed: int = SAMPLE_SEED, n_reads: int = 2000, length: int = N_LEN):
    """(reads, planted junctions as (cell, D, frequency)): random reads of both strands of the genome, each planted junction and
    the short deletion present in a read with its frequency, 0.5 % of the bases substituted; 2 % of the reads jump
    backward, 2 % carry six substitutions more."""
    rng = random.Random(seed)
    planted = [(_free_pos(g, lo, d), d, af) for lo, d, af in PLANTED]
    short = (_free_pos(g, SHORT[0], SHORT[1]), SHORT[1], SHORT[2])
    reads = []
    for _ in range(n_reads):
        start = rng.randrange(SAMPLE_SPAN[0], SAMPLE_SPAN[1])
        dels = {p: d for p, d, af in planted + [short] if rng.random() < af}
        out, i = [], start
        while len(out) < length:
            if i in dels:
                i += dels.pop(i)
                continue
            out.append(g[i])
            i += 1
        kind = rng.random()
        if kind < 0.02:
            half = length // 2
            out = list(g[start + 200:start + 200 + half] + g[start:start + length - half])
        for o in range(length):
            if rng.random() < 0.005:
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
        if 0.02 <= kind < 0.04:
            for o in rng.sample(range(length // 3, 2 * length // 3), 6):
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
        r = "".join(out)
        reads.append(junctions_ref.revcomp(r) if rng.random() < 0.5 else r)
    return reads, planted
