"""Inputs of the duplication tests (tests/test_duplications_cpu.py, tests/test_gpu_duplications.py): crafted records on the junction
tests' crafted genome with one sequence more, and a sample of random reads of a genome with planted tandem duplications and reads
across its origin.  What the rule makes of them is duplications_ref's business."""
from __future__ import annotations

import random

from tests import duplications_ref, junction_cases
from tests.indel_cases import _rand, mut_read
from tests.junction_cases import _set

N_LEN = 150
ND = (400, 410)     # craftD's run of N


def crafted_genome(k: int):
    """junction_cases.crafted_genome(k) -- craftA (a homopolymer run, a dinucleotide repeat, a repeat of k + 24 bases, a stretch of N
    [1300, 1320)), craftB, craftC (three stretches that occur twice, of exactly 1, 6 and k - 1 bases) -- and behind them craftD: random
    letters with a run of N [400, 410) whose first k - 1 letters behind the run's first, [411, 410 + k), are those of [111, 110 + k);
    the letters in front of the two copies ([410] and [110]) and behind them differ.  The other sequences' cells stay where they are."""
    rng = random.Random(3000 + k)
    d = list(_rand(rng, 900))
    d[ND[0]:ND[1]] = "N" * (ND[1] - ND[0])
    d[ND[0] - 1] = "G"                               # (the index reads N as A: no homopolymer k-mer of A's around the run)
    d[ND[1] + 1:ND[1] + k] = d[111:110 + k]
    for u, v in ((110, ND[1]), (110 + k, ND[1] + k)):
        d[v] = "ACGT"[("ACGT".index(d[u]) + 1) % 4]
    return junction_cases.crafted_genome(k) + [("craftD", "".join(d))]


def dup_read(ref: str, pos: int, e: int, left: int = 75, n: int = N_LEN, subs=()):
    """A read across the junction of the two copies of a tandem duplication of ref[pos - e, pos): `left` bases up to cell pos - 1,
    then on from cell pos - e; the read's offsets `subs` changed to another base."""
    out = list(ref[pos - left:pos] + ref[pos - e:pos - e + n - left])
    assert len(out) == n and pos - left >= 0
    for o in subs:
        out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
    return "".join(out)


def origin_read(seq: str, left: int, right: int) -> str:
    """The last `left` and the first `right` bases of a circular sequence"""
    return seq[len(seq) - left:] + seq[:right]


def free_pos(ref: str, lo: int, e: int) -> int:
    """The first cell >= lo at which a duplication of e cannot slide to the left"""
    p = lo
    while ref[p - 1] == ref[p - e - 1]:
        p += 1
    return p


def haplotype(text: str, cell: int, e: int) -> str:
    """The genome with text[cell - e, cell) there twice"""
    return text[:cell] + text[cell - e:]


def half(k: int) -> int:
    """The bases on either side of the junction in the short records: 32 at k = 21"""
    return k + 11


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(k); every read is there along and against the reference (label + '/rc').
    expect, at min_len 33 and 2 mismatches: ('dup', cell, E) the event the record supports as planted (before normalisation), 'span',
    'short', 'forward', 'discordant', 'none' for a record that leaves no tally behind `anchored`, or None (not looked at one by one)."""
    (_, a), (_, b), (_, c), (_, d) = crafted_genome(k)
    first_b, first_c, first_d = len(a), len(a) + len(b), len(a) + len(b) + len(c)
    text = a + b + c + d
    n, hf = N_LEN, half(k)
    cases = []

    # junction-only reads: 2 (k + 11) bases do not hold a copy of 33; the longer ones 150 bases
    for e in (33, 34):
        pos = free_pos(a, 900, e)
        cases.append(("e%d" % e, dup_read(a, pos, e, hf, 2 * hf), ("dup", pos, e)))
    for e in (64, 200, 1000):
        pos = free_pos(a, 1200, e)
        cases.append(("e%d" % e, dup_read(a, pos, e), ("dup", pos, e)))
    p33, p200 = free_pos(a, 900, 33), free_pos(a, 1200, 200)
    cases.append(("whole_copy_33", dup_read(a, p33, 33), ("dup", p33, 33)))                   # ... and 150 bases hold a whole second copy
    cases.append(("two_whole_copies_33", a[p33 - 50:p33] + a[p33 - 33:p33] + a[p33 - 33:p33 + 34], None))   # three copies: two jumps in one read
    # the origin of a circular sequence: craftB (the second sequence), craftD (the last: pos = the index's cells), a read of 150
    cases.append(("origin_b", origin_read(b, hf, hf), ("dup", first_b + len(b), len(b))))
    cases.append(("origin_d", origin_read(d, hf, hf), ("dup", first_d + len(d), len(d))))
    cases.append(("origin_b_150", origin_read(b, 70, 80), ("dup", first_b + len(b), len(b))))
    cases.append(("origin_b_sub", _set(origin_read(b, 70, 80), 72, "ACGT"[("ACGT".index(b[2]) + 1) % 4]), ("dup", first_b + len(b), len(b))))
    # only p0 clipped: the right arm begins at the sequence's first cell, the left arm ends inside it; only p1: the reverse
    eb = next(e for e in range(200, 400) if b[e - 1] == a[-1])         # (the letter in front of craftB's first is craftA's last: F_R stops the slide)
    cases.append(("starts_at_first_cell", b[eb - 75:eb] + b[:75], ("dup", first_b + eb, eb)))
    yb = next(y for y in range(300, 500) if b[-1] != b[y - 1])
    cases.append(("ends_at_last_cell", b[len(b) - 75:] + b[yb:yb + 75], ("dup", first_b + len(b), len(b) - yb)))
    # an overhang beyond the sequence: eight foreign bases in front of craftA's first cells (dL < lo), behind craftB's last (dR + n > hi)
    x8 = "ACCAGTCA"
    cases.append(("overhang_front", x8 + a[:70] + a[20:92], "none"))
    cases.append(("overhang_front_b", x8 + b[:70] + b[20:92], "none"))
    cases.append(("overhang_back", b[len(b) - 70:len(b) - 20] + b[len(b) - 92:] + x8, "none"))
    cases.append(("no_overhang_front", a[:78] + a[20:92], ("dup", 78, 58)))
    # the anchors in two sequences, either way round
    cases.append(("a_and_b", a[700:775] + b[100:175], "none"))
    cases.append(("b_and_a", b[100:175] + a[700:775], "none"))
    # craftA's run of N [1300, 1320).  The left arm's cells are [dL, dL + b), b = n - k the back anchor's offset: the run's first cell
    # the arm's last, and just behind it.  The right arm's are [dR + k, dR + n): the run's last cell the arm's first, and just in front.
    bk = n - k
    for label, dl, expect in (("n_last_of_left_arm", 1301 - bk, "none"), ("n_behind_left_arm", 1300 - bk, "dup")):
        pos = dl + 75
        cases.append((label, dup_read(a, pos, 400), ("dup", pos, 400) if expect == "dup" else "none"))
    for label, dr, expect in (("n_first_of_right_arm", 1319 - k, "none"), ("n_in_front_of_right_arm", 1320 - k, "dup")):
        pos = dr + 33 + 75
        cases.append((label, dup_read(a, pos, 33), ("dup", pos, 33) if expect == "dup" else "none"))
    cases.append(("n_in_left_arm", a[1262:1337].replace("N", "A") + a[900:975], "none"))
    # normalisation.  By a letter: the flanks share 1, 6, k - 1 bases (craftC), the record breaks in the middle of the shared stretch.
    for label, (x, y, h) in junction_cases.homology_sites(k).items():
        bp = y + (h + 1) // 2
        cases.append(("homology_" + label, dup_read(c, bp, y - x), ("dup", first_c + bp, y - x)))
    # By F_R behind the run of N, whose cells the engine's reference holds as A: the duplicated stretch begins at the run's end and ends
    # in A (the record breaks right behind its front anchor: the right arm begins k bases in front of the breakpoint at the latest)
    en = next(e for e in range(40, 170) if a[1320 + e - 1] == "A")
    cases.append(("floor_right_at_n", dup_read(a, 1320 + en, en, k), ("dup", 1320 + en, en)))
    # By F_L: craftD's [411, 410 + k) are [111, 110 + k); the front anchor is the stretch's first k-mer and the record breaks right behind it
    cases.append(("floor_left_at_n", d[ND[1]:ND[1] + k] + d[110 + k:110 + k + n - k], ("dup", first_d + ND[1] + k, 300)))
    cases.append(("in_homopolymer", dup_read(a, 306, 100), None))
    cases.append(("in_dinucleotide", dup_read(a, 1210, 700), None))
    # substitutions
    plain = dup_read(a, p200, 200)
    cases.append(("m_eq_M", dup_read(a, p200, 200, subs=(40, 100)), ("dup", p200, 200)))
    cases.append(("m_eq_M_plus_1", dup_read(a, p200, 200, subs=(40, 60, 100)), "discordant"))
    cases.append(("sub_left_of_bp", _set(plain, 74, a[p200 - 200 - 1]), ("dup", p200 - 1, 200)))
    cases.append(("anchor_try2_front", dup_read(a, p200, 200, subs=(3,)), ("dup", p200, 200)))
    cases.append(("anchor_try2_back", dup_read(a, p200, 200, subs=(n - 4,)), ("dup", p200, 200)))
    cases.append(("bp_at_a_plus_k", dup_read(a, p200, 200, k), ("dup", p200, 200)))
    cases.append(("bp_at_b", dup_read(a, p200, 200, n - k), ("dup", p200, 200)))
    cases.append(("bp_in_last_k", dup_read(a, p200, 200, n - k + 5), None))
    cases.append(("n_2k", dup_read(a, p200, 200, k, 2 * k), ("dup", p200, 200)))
    cases.append(("n_2k_minus_1", dup_read(a, p200, 200, k, 2 * k - 1), "none"))
    # forty foreign bases between two halves that follow each other: delta = -40, discordant by its mismatches
    rng = random.Random(77)
    cases.append(("inserted_40", a[800:855] + _rand(rng, 40) + a[855:910], "discordant"))
    for e in (32, 17, 1):
        pos = free_pos(a, 950, e)
        cases.append(("e%d" % e, dup_read(a, pos, e), "short"))
    cases.append(("deletion_400", mut_read(a, 690, n, dele=(760, 400)), "forward"))
    cases.append(("deletion_1", mut_read(a, 690, n, dele=(free_pos(a, 760, 1), 1)), "forward"))
    cases.append(("plain", a[p200 - 70:p200 + 80], "span"))
    cases.append(("plain_at_first_cells", b[:n], "span"))
    cases.append(("plain_at_last_cells", d[len(d) - n:], "span"))
    cases.append(("plain_mismatches", mut_read(a, 900, n, subs=(40, 60, 100)), "discordant"))
    out = []
    for label, read, expect in cases:
        assert set(read) <= set("ACGT"), label
        out.append((label, read, expect))
        out.append((label + "/rc", duplications_ref.revcomp(read), expect))
    return out, text


SAMPLE_SEED = 1
SAMPLE_SPAN = (800, 6800)          # the planted duplications end in these cells of the genome


def planted(g: str, seed: int = SAMPLE_SEED, n_sites: int = 40):
    """(cell, E) of the sample's duplications: four that many reads carry, the rest one or two reads each"""
    rng = random.Random(1000 + seed)
    out = [(free_pos(g, 1500, 33), 33), (free_pos(g, 2500, 150), 150), (free_pos(g, 4000, 1200), 1200), (free_pos(g, 6000, 47), 47)]
    while len(out) < n_sites:
        e = rng.choice((33, 34, 40, 64, 100, 333, 700))
        out.append((free_pos(g, rng.randrange(max(SAMPLE_SPAN[0], e + 200), SAMPLE_SPAN[1]), e), e))
    return out


def sample_reads(g: str, seed: int = SAMPLE_SEED, n_reads: int = 2000, length: int = N_LEN):
    """(reads, the four frequent duplications as (cell, E)): random reads of both strands of a circular genome.  Of a hundred reads
    about 20 cross the junction of one of the four frequent duplications, 4 of one of the rare ones, 4 the origin, 3 jump backward
    by 1 to 32 bases, 3 forward (a deletion), 3 carry six substitutions more, 2 a stretch of foreign bases; the rest are plain.
    0.5 % of the bases are substituted."""
    rng = random.Random(seed)
    sites = planted(g, seed)
    reads = []
    lo_left = min(30, length // 2)
    for _ in range(n_reads):
        kind = rng.random()
        left = rng.randrange(lo_left, length - lo_left + 1)
        if kind < 0.24:
            pos, e = sites[rng.randrange(4)] if kind < 0.20 else sites[rng.randrange(4, len(sites))]
            out = g[pos - left:pos] + g[pos - e:pos - e + length - left]
        elif kind < 0.28:
            out = origin_read(g, left, length - left)
        elif kind < 0.31:
            pos, e = rng.randrange(*SAMPLE_SPAN), rng.randrange(1, 33)
            out = g[pos - left:pos] + g[pos - e:pos - e + length - left]
        elif kind < 0.34:
            start = rng.randrange(*SAMPLE_SPAN)
            out = mut_read(g, start, length, dele=(start + left, rng.choice((1, 7, 33, 500))))
        elif kind < 0.36:
            start = rng.randrange(*SAMPLE_SPAN)
            out = g[start:start + left] + _rand(rng, 40) + g[start + left:]
        else:
            start = rng.randrange(*SAMPLE_SPAN)
            out = g[start:start + length]
        out = list(out[:length])
        assert len(out) == length
        for o in range(length):
            if rng.random() < 0.005:
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
        if 0.36 <= kind < 0.39:
            for o in rng.sample(range(length // 3, 2 * length // 3), 6):
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
        r = "".join(out)
        reads.append(duplications_ref.revcomp(r) if rng.random() < 0.5 else r)
    return reads, sites[:4]
