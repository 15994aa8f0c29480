"""Inputs of the breakend tests (tests/test_breakends_cpu.py, tests/test_gpu_breakends.py): crafted records on a small genome of three
sequences, and samples of random reads that leave the reference.  What the rule makes of them is breakends_ref's business."""
from __future__ import annotations

import random

from tests.breakends_ref import L, R, revcomp

N_RUN = (600, 620)      # bkB's run of N
REPEAT = (200, 700, 60)   # bkC[200:260] == bkC[700:760]: no anchor k-mer inside either copy
EDGE = 6                # clipped bases that continue into the neighbouring sequence / the run of N (read as A)


def _rand(rng, n: int) -> str:
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(c: str, *avoid: str) -> str:
    return next(x for x in "ACGT" if x != c and x not in avoid)


def crafted_genome():
    """[(name, letters)]: bkA random; bkB, the middle one, random with the run N_RUN; bkC random with the repeat REPEAT"""
    rng = random.Random(5150)
    a, b, c = _rand(rng, 1500), list(_rand(rng, 1200)), list(_rand(rng, 1300))
    b[N_RUN[0] - 1:N_RUN[1] + 1] = "G" + "N" * (N_RUN[1] - N_RUN[0]) + "C"
    u, v, h = REPEAT
    c[v:v + h] = c[u:u + h]
    return [("bkA", a), ("bkB", "".join(b)), ("bkC", "".join(c))]


def foreign(rng, n: int, avoid_head: str = "", avoid_tail: str = "") -> str:
    """n random bases; the first ones differ base by base from avoid_head, the last ones from avoid_tail (aligned at the end): what the
    reference has beyond the breakpoint, so that no walk goes on into the clipped bases by chance"""
    s = list(_rand(rng, n))
    for i, c in enumerate(avoid_head[:n]):
        if s[i] == c:
            s[i] = _other(c)
    for i, c in enumerate(reversed(avoid_tail[-n:] if avoid_tail else "")):
        if s[n - 1 - i] == c:
            s[n - 1 - i] = _other(c)
    return "".join(s)


def _idx(text: str) -> str:
    return "".join(c if c in "ACGT" else "A" for c in text)


def sub(read: str, *offsets: int) -> str:
    out = list(read)
    for o in offsets:
        out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
    return "".join(out)


def breakend_read(text: str, cell: int, side: int, held: int, clip: str) -> str:
    """r' of a read that holds `held` cells up to (L) or from (R) `cell` and goes on with the bases `clip`"""
    if side == L:
        assert cell - held + 1 >= 0
        return _idx(text[cell - held + 1:cell + 1]) + clip
    return clip + _idx(text[cell:cell + held])


def clipped(text: str, rng, cell: int, side: int, n: int, clip: int) -> str:
    """... with `clip` foreign bases whose base next to the breakpoint is not the reference's"""
    if side == L:
        return breakend_read(text, cell, L, n - clip, foreign(rng, clip, avoid_head=_idx(text[cell + 1:cell + 9])))
    return breakend_read(text, cell, R, n - clip, foreign(rng, clip, avoid_tail=_idx(text[max(0, cell - 8):cell])))


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(); every read is there as it is and reverse-complemented (label + '/rc').
    expect, at min_clip 20 and 2 mismatches: ('be', cell, side) the site the record supports, the name of the one tally of a
    one_anchor record, 'span', 'nothing' for a record that leaves no tally behind `records`, None where the test asks more."""
    seqs = crafted_genome()
    text = "".join(s for _, s in seqs)
    fa, fb, fc = 0, len(seqs[0][1]), len(seqs[0][1]) + len(seqs[1][1])
    end = len(text)
    rng = random.Random(77 + k)
    n = 64
    cases = []
    x, y = fa + 400, fa + 800                        # a site held from below and one held from above
    for side, cell, name in ((L, x, "L"), (R, y, "R")):
        mid = n - 30 if side == L else 29            # a substitution that breaks the far end's third and fourth k-mer: clips below 25
        cases.append((name + "_plain", clipped(text, rng, cell, side, n, 25), ("be", cell, side)))
        cases.append((name + "_150", clipped(text, rng, cell, side, 150, 40), ("be", cell, side)))
        cases.append((name + "_300", clipped(text, rng, cell, side, 300, 100), ("be", cell, side)))
        for clip, what in ((19, "short"), (20, ("be", cell, side)), (21, ("be", cell, side)), (16, "short")):
            cases.append(("%s_clip_%d" % (name, clip), sub(clipped(text, rng, cell, side, n, clip), mid), what))
        cases.append((name + "_clip_16_no_substitution", clipped(text, rng, cell, side, n, 16), "nothing"))   # two anchors, the clip as mismatches
        # a mismatch 5 bases before the breakpoint is followed by 4 matches: the tie, the walk stays in front of it; 6 before: crossed
        bp = n - 25 if side == L else 25             # p* (q*) of the unbroken read
        tie, ext = (bp - 5, bp - 6) if side == L else (bp + 4, bp + 5)
        moved = cell - 5 if side == L else cell + 5
        cases.append((name + "_mismatch_then_4", sub(clipped(text, rng, cell, side, n, 25), tie), ("be", moved, side)))
        cases.append((name + "_mismatch_then_5", sub(clipped(text, rng, cell, side, n, 25), ext), ("be", cell, side)))
        # foreign bases that continue the reference by 1 to 3 bases are held
        for e in (1, 2, 3):
            to = cell + e if side == L else cell - e
            cases.append(("%s_continues_%d" % (name, e), clipped(text, rng, to, side, n, 25), ("be", to, side)))
        # the anchor at the second, third and fourth offset: the mismatches in front of it count
        long = clipped(text, rng, cell, side, 150, 40)
        at = (lambda o: o) if side == L else (lambda o: 149 - o)
        cases.append((name + "_anchor_try2", sub(long, at(3)), ("be", cell, side)))
        cases.append((name + "_anchor_try3", sub(long, at(3), at(10)), ("be", cell, side)))
        cases.append((name + "_anchor_try4", sub(long, at(3), at(10), at(18)), "discordant"))
        short = clipped(text, rng, cell, side, n, 25)
        at = (lambda o: o) if side == L else (lambda o: n - 1 - o)
        cases.append((name + "_m_eq_M", sub(short, at(3), at(5)), ("be", cell, side)))
        cases.append((name + "_m_eq_M_plus_1", sub(short, at(3), at(5), at(7)), "discordant"))
        # two tags at one cell, and two that differ in one base
        tag = clipped(text, rng, cell, side, n, 25)
        cases.append((name + "_second_tag", tag, ("be", cell, side)))
        cases.append((name + "_tag_one_base_apart", sub(tag, n - 12 if side == L else 12), ("be", cell, side)))
        # n = 2k - 1 and 2k; the lengths around ten and sixteen words of a packed record
        cases.append((name + "_n_2k", clipped(text, rng, cell, side, 2 * k, k), ("be", cell, side)))
        cases.append((name + "_n_2k_minus_1", clipped(text, rng, cell, side, 2 * k - 1, k - 1), "nothing"))
        for ln in (159, 160, 161, 255, 256, 257):
            cases.append(("%s_n_%d" % (name, ln), clipped(text, rng, cell, side, ln, 40), ("be", cell, side)))
    # the termini of the middle sequence: the clipped bases go on as the neighbouring sequence does, the walk stops at the border
    cases.append(("last_cell_of_b", breakend_read(text, fc - 1, L, n - 25, text[fc:fc + EDGE] + foreign(rng, 25 - EDGE, avoid_head=text[fc + EDGE:fc + EDGE + 8])), ("be", fc - 1, L)))
    cases.append(("first_cell_of_b", breakend_read(text, fb, R, n - 25, foreign(rng, 25 - EDGE, avoid_tail=text[fb - EDGE - 8:fb - EDGE]) + text[fb - EDGE:fb]), ("be", fb, R)))
    cases.append(("first_cell_of_a", clipped(text, rng, fa, R, n, 25), ("be", fa, R)))
    cases.append(("last_cell_of_c", clipped(text, rng, end - 1, L, n, 25), ("be", end - 1, L)))
    # ... and at the run of N, whose cells the index holds as A (so that a k-mer that runs on into them with A is an anchor: the far
    # end's four k-mers each hold a foreign base)
    n0, n1 = fb + N_RUN[0], fb + N_RUN[1]
    cases.append(("stops_below_n_run", breakend_read(text, n0 - 1, L, n - 25 - EDGE, "A" * EDGE + foreign(rng, 25, avoid_head="A" * 8)), ("be", n0 - 1, L)))
    cases.append(("stops_above_n_run", breakend_read(text, n1, R, n - 25 - EDGE, foreign(rng, 25, avoid_tail="A" * 8) + "A" * EDGE), ("be", n1, R)))
    # unplaced: the held end runs off its stretch (the anchor is the second try: eight bases hang over the border); the anchor lies over N
    cases.append(("d_below_lo", foreign(rng, 8) + _idx(text[fb:fb + 31]) + foreign(rng, 25, avoid_head=text[fb + 31:fb + 39]), "unplaced"))
    cases.append(("d_plus_n_above_hi", foreign(rng, 25, avoid_tail=text[fc - 39:fc - 31]) + text[fc - 31:fc] + foreign(rng, 8), "unplaced"))
    cases.append(("d_below_lo_at_n_run", foreign(rng, 8) + _idx(text[n1:n1 + 31]) + foreign(rng, 25, avoid_head=text[n1 + 31:n1 + 39]), "unplaced"))
    cases.append(("anchor_over_n_L", _idx(text[n0 - 10:n0 - 10 + k]) + foreign(rng, n - k), "unplaced"))
    cases.append(("anchor_over_n_R", foreign(rng, n - k) + _idx(text[n1 + 10 - k:n1 + 10]), "unplaced"))
    # clip = 0: the far end lies in a repeat, where no k-mer is an anchor
    u, v, h = REPEAT
    assert h >= k + 24
    cases.append(("through_repeat_L", text[fc + u + k + 24 - n:fc + u + k + 24], "through"))
    cases.append(("through_repeat_R", text[fc + v + h - k - 24:fc + v + h - k - 24 + n], "through"))
    # records of two anchors and of none leave nothing; plain records count for the span
    cases.append(("deletion", text[fa + 700:fa + 732] + text[fa + 1100:fa + 1132], "nothing"))
    cases.append(("chimera", text[fa + 700:fa + 732] + text[fc + 1000:fc + 1032], "nothing"))
    cases.append(("foreign", foreign(rng, n), "nothing"))
    cases.append(("plain_over_x", text[x - 30:x + 34], "span"))
    cases.append(("plain_over_y", text[y - 75:y + 75], "span"))
    cases.append(("plain_b", text[fb + 100:fb + 400], "span"))
    cases.append(("plain_mismatches", sub(text[fa + 900:fa + 964], 28, 32, 36), "nothing"))
    out = []
    for label, read, expect in cases:
        assert set(read) <= set("ACGT"), label
        out.append((label, read, expect))
        out.append((label + "/rc", revcomp(read), expect))
    return out, text


# ---- a sample of random reads ------------------------------------------------------------------------------------------------------
FUZZ_SEED = 11
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def fuzz_genome(seed: int):
    """[(name, letters)] of three to five sequences of 1,200 to 2,500 random letters, a run of N in the first, a repeat of 80 bases
    inside the second"""
    rng = random.Random(seed)
    seqs = [list(_rand(rng, rng.randrange(1200, 2501))) for _ in range(rng.randrange(3, 6))]
    at = rng.randrange(400, 800)
    seqs[0][at:at + 15] = "N" * 15
    seqs[1][900:980] = seqs[1][300:380]
    return [("fuzz%d" % i, "".join(s)) for i, s in enumerate(seqs)]


def fuzz_reads(seqs, seed: int, n_reads: int, k: int = 21, lengths=(64, 150), one_anchor: float = 0.5):
    """Random reads: a share `one_anchor` of them leave the reference -- at one of 40 sites or at a random cell, also near the
    borders and the run of N, the clipped bases random, one of three shared stretches, or an adapter, with 0 to 3 substitutions
    in the held part; of the rest most are plain reads with 0.5 % of their bases substituted, some carry a deletion, some are
    foreign.  Half of all reads are reverse-complemented."""
    rng = random.Random(seed)
    text = "".join(s for _, s in seqs)
    first = [0]
    for _, s in seqs:
        first.append(first[-1] + len(s))
    sites = [(rng.randrange(len(text)), rng.choice((L, R))) for _ in range(40)]
    sites += [(first[1], R), (first[1] - 1, L), (first[2], R), (len(text) - 1, L), (0, R)]
    shared = [_rand(rng, 200) for _ in range(3)]
    reads = []
    while len(reads) < n_reads:
        n = rng.randrange(lengths[0], lengths[1] + 1)
        u = rng.random()
        if u < one_anchor:
            cell, side = rng.choice(sites) if rng.random() < 0.7 else (rng.randrange(len(text)), rng.choice((L, R)))
            held = rng.randrange(k, n - 15)
            if (side == L and cell - held + 1 < 0) or (side == R and cell + held > len(text)):
                continue
            v = rng.random()
            tail = rng.choice(shared)[:n - held] if v < 0.5 else ADAPTER[:n - held] + _rand(rng, max(0, n - held - len(ADAPTER))) if v < 0.6 else _rand(rng, n - held)
            r = breakend_read(text, cell, side, held, tail if side == L else tail[::-1])
            r = sub(r, *rng.sample(range(n), rng.choice((0, 0, 0, 1, 2, 3))))
        elif u < one_anchor + 0.05:
            r = _rand(rng, n)
        else:
            start = rng.randrange(0, len(text) - n - 45)
            out = list(text[start:start + n])
            if u < one_anchor + 0.12:                              # a deletion of 5 to 40 bases
                cut = rng.randrange(5, 41)
                out = list(text[start:start + n // 2] + text[start + n // 2 + cut:start + n + cut])
            for o in range(n):
                if rng.random() < 0.005 and out[o] != "N":
                    out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
            r = _idx("".join(out))
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    return reads


def fuzz_world(seed: int = FUZZ_SEED, n_reads: int = 2000, k: int = 21):
    """([(name, letters)] of fuzz_genome(seed), reads of 64 to 150 bases, half of them leaving the reference)"""
    seqs = fuzz_genome(seed)
    return seqs, fuzz_reads(seqs, seed + 2, n_reads, k)
