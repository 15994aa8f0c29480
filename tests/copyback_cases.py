"""Inputs of the copy-back tests (tests/test_copybacks_cpu.py, tests/test_gpu_copybacks.py): crafted records on the junction tests'
crafted genome with one more sequence, and samples of random reads with strand switches.  What the rule makes of them is
copybacks_ref's business."""
from __future__ import annotations

import random

from tests import junction_cases
from tests.copybacks_ref import H, T, revcomp
from tests.indel_cases import _rand

N_LEN = 150
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def turn_sites(k: int):
    """label -> (u, v, h), offsets in craftD: the h letters from u on are the reverse complement of the h letters that end at v, and
    the letters around them are not.  A kind-H turn (x, y) = (u - 1, v) and a kind-T turn (x, y) = (u, v + 1) can slide h steps up."""
    return {"one": (200, 560, 1), "six": (300, 700, 6), "k_minus_1": (400, 830, k - 1)}


HAIRPIN = (1000, 6)     # craftD[1000:1006] is its own reverse complement: a hairpin's slide crosses x = y there
N_RUN = (900, 920)      # craftD's run of N


def crafted_genome(k: int):
    """junction_cases.crafted_genome(k) -- craftA, craftB, craftC, their cells where they are -- and behind them craftD: random
    letters with turn_sites' three pairs of stretches, the palindrome HAIRPIN and the run N_RUN."""
    rng = random.Random(3000 + k)
    d = list(_rand(rng, 1200))
    for (u, v, h) in turn_sites(k).values():
        d[u:u + h] = revcomp("".join(d[v - h + 1:v + 1]))
        for p, q in ((u - 1, v + 1), (u + h, v - h)):           # the run ends on both sides
            d[q] = "ACGT"[("ACGT".index(_COMP[d[p]]) + 1) % 4]
    c, w = HAIRPIN
    d[c + w // 2:c + w] = revcomp("".join(d[c:c + w // 2]))
    d[c + w] = "ACGT"[("ACGT".index(_COMP[d[c - 1]]) + 1) % 4]
    d[N_RUN[0] - 1:N_RUN[1] + 1] = "G" + "N" * (N_RUN[1] - N_RUN[0]) + "G"
    return junction_cases.crafted_genome(k) + [("craftD", "".join(d))]


def turn_read(ref: str, kind: int, x: int, y: int, la: int = N_LEN // 2, lb: int = N_LEN - N_LEN // 2, subs=()) -> str:
    """A read that turns at the pair of cells (x, y) of `ref`: la bases of arm A that end at the base of cell x, lb bases of arm B
    that begin at the base of cell y.  Kind H runs up to x and comes back down from y; kind T runs down to x and goes up from y.
    Letters that are not ACGT read as A; the offsets `subs` are changed to another base."""
    if kind == H:
        r = ref[x - la + 1:x + 1] + revcomp(ref[y - lb + 1:y + 1].replace("N", "A"))
    else:
        r = revcomp(ref[x:x + la].replace("N", "A")) + ref[y:y + lb]
    out = list(r.replace("N", "A"))
    assert len(out) == la + lb
    for o in subs:
        out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
    return "".join(out)


def _slides(ref, kind, x, y):
    if kind == H:
        return ref[x + 1] == _COMP[ref[y]] or ref[x] == _COMP[ref[y + 1]]
    return _COMP[ref[x]] == ref[y - 1] or _COMP[ref[x - 1]] == ref[y]


def free_pair(ref: str, kind: int, x: int, y: int):
    """The first pair (x, y' >= y) that cannot slide either way"""
    while _slides(ref, kind, x, y):
        y += 1
    return x, y


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(k); every read is there as it is and reverse-complemented (label + '/rc').
    expect, at 2 mismatches: ('cb', kind, lo, hi) the event the record supports, 'span', 'discordant', 'none' for a record that
    leaves no tally behind `switched` or `same_strand`, or None where only the agreement of the implementations is asked."""
    seqs = crafted_genome(k)
    text = "".join(s for _, s in seqs)
    a = seqs[0][1]
    first_c = len(seqs[0][1]) + len(seqs[1][1])
    first_d = first_c + len(seqs[2][1])
    end_d = len(text)
    n, half = N_LEN, N_LEN // 2
    cases = []

    def cb(kind, x, y):
        return ("cb", kind, min(x, y), max(x, y))

    for kind, name in ((H, "H"), (T, "T")):
        x, y = free_pair(text, kind, first_d + 140, first_d + 480)
        plain = turn_read(text, kind, x, y)
        cases.append((name + "_plain", plain, cb(kind, x, y)))
        xb, yb = free_pair(text, kind, first_d + 640, first_d + 130)       # arm B's turn below arm A's
        cases.append((name + "_y_below_x", turn_read(text, kind, xb, yb), cb(kind, xb, yb)))
        cases.append((name + "_bp_at_f_plus_k", turn_read(text, kind, x, y, k, n - k), cb(kind, x, y)))
        cases.append((name + "_bp_at_g", turn_read(text, kind, x, y, n - k, k), cb(kind, x, y)))
        cases.append((name + "_bp_in_last_k", turn_read(text, kind, x, y, n - k + 5, k - 5), None))
        cases.append((name + "_bp_in_first_k", turn_read(text, kind, x, y, k - 5, n - k + 5), None))
        cases.append((name + "_n_2k", turn_read(text, kind, x, y, k, k), cb(kind, x, y)))
        cases.append((name + "_n_2k_minus_1", turn_read(text, kind, x, y, k, k - 1), "none"))
        cases.append((name + "_n_64", turn_read(text, kind, x, y, 32, 32), cb(kind, x, y)))
        xw, yw = free_pair(text, kind, first_d + 450, first_d + 710)
        cases.append((name + "_n_300", turn_read(text, kind, xw, yw, 170, 130), cb(kind, xw, yw)))
        cases.append((name + "_sub_at_p_minus_1", turn_read(text, kind, x, y, subs=(half - 1,)), None))
        cases.append((name + "_sub_at_p", turn_read(text, kind, x, y, subs=(half,)), None))
        cases.append((name + "_m_eq_M", turn_read(text, kind, x, y, subs=(40, 100)), cb(kind, x, y)))
        cases.append((name + "_m_eq_M_plus_1", turn_read(text, kind, x, y, subs=(40, 60, 100)), "discordant"))
        cases.append((name + "_anchor_try2_front", turn_read(text, kind, x, y, subs=(3,)), cb(kind, x, y)))
        cases.append((name + "_anchor_try2_back", turn_read(text, kind, x, y, subs=(n - 4,)), cb(kind, x, y)))
        # each palindrome length: the record turns in the middle of the shared stretch (at its end for one base)
        for label, (u, v, h) in turn_sites(k).items():
            x0, y0 = (first_d + u - 1, first_d + v) if kind == H else (first_d + u, first_d + v + 1)
            t = (h + 1) // 2
            cases.append(("%s_palindrome_%s" % (name, label), turn_read(text, kind, x0 + t, y0 - t), cb(kind, x0, y0)))
        # a hairpin where the reference is no palindrome: hi = lo
        xh = first_d + 250
        while _slides(text, kind, xh, xh):
            xh += 1
        cases.append((name + "_hairpin", turn_read(text, kind, xh, xh), cb(kind, xh, xh)))
        # a hairpin in the palindrome: the run of pairs crosses x = y and ends at the same two cells on either side
        c, w = first_d + HAIRPIN[0], HAIRPIN[1]
        if kind == H:
            cases.append((name + "_hairpin_palindrome", turn_read(text, kind, c + w // 2 - 1, c + w // 2 - 1), cb(kind, c - 1, c + w - 1)))
            cases.append((name + "_hairpin_palindrome_off_centre", turn_read(text, kind, c + 1, c + w - 3), cb(kind, c - 1, c + w - 1)))
        else:
            cases.append((name + "_hairpin_palindrome", turn_read(text, kind, c + w // 2, c + w // 2), cb(kind, c, c + w)))
            cases.append((name + "_hairpin_palindrome_off_centre", turn_read(text, kind, c + 2, c + w - 2), cb(kind, c, c + w)))
    # arms that end at the last and at the first cell of a sequence are found.  (Arm A's cells are those of the offsets in front of
    # the back anchor, arm B's those behind the front anchor: a turn at a sequence's border is found where the anchor beyond it ends
    # at the turn, and ignored one base further in.)
    last = end_d - 1
    yl = first_d + 300
    while text[last] == _COMP[text[yl + 1]]:                       # no step down from (last, yl); none up, the sequence ends
        yl += 1
    cases.append(("H_arm_a_ends_at_last_cell", turn_read(text, H, last, yl, n - k, k), cb(H, last, yl)))
    cases.append(("H_arm_a_ends_at_last_cell_p_below_g", turn_read(text, H, last, yl, n - k - 1, k + 1), "none"))
    xl = first_d + 300
    while text[xl + 1] == _COMP[text[last]]:                       # arm B comes down from the last cell: no step down; none up either
        xl += 1
    cases.append(("H_arm_b_begins_at_last_cell", turn_read(text, H, xl, last, k, n - k), cb(H, xl, last)))
    yf = first_d + 400
    while _COMP[text[first_d]] == text[yf - 1]:
        yf += 1
    cases.append(("T_arm_a_ends_at_first_cell", turn_read(text, T, first_d, yf, n - k, k), cb(T, first_d, yf)))
    xf = first_d + 400
    while _COMP[text[xf - 1]] == text[first_d]:
        xf += 1
    cases.append(("T_arm_b_begins_at_first_cell", turn_read(text, T, xf, first_d, k, n - k), cb(T, first_d, xf)))
    cases.append(("T_arm_b_begins_at_first_cell_p_above_f_plus_k", turn_read(text, T, xf, first_d, k + 1, n - k - 1), "none"))
    # the arms' far ends at a sequence's border: the read itself begins or ends there
    x, y = free_pair(text, H, first_d + half - 1, first_d + 480)
    cases.append(("H_arm_a_begins_at_first_cell", turn_read(text, H, x, y), cb(H, x, y)))
    x0, y0 = first_d + 480, first_d + (n - half) - 1
    while _slides(text, H, x0, y0):
        x0 += 1
    cases.append(("H_arm_b_ends_at_first_cell", turn_read(text, H, x0, y0), cb(H, x0, y0)))
    x, y = free_pair(text, T, last - half + 1, first_d + 480)
    cases.append(("T_arm_a_begins_at_last_cell", turn_read(text, T, x, y), cb(T, x, y)))
    # an arm that would leave the sequence: arm B of a kind-H record comes down through craftD's first cell into craftC's letters,
    # and the back anchor is the third try, inside craftD
    cases.append(("arm_leaves_sequence", turn_read(text, H, first_d + 500, first_d + 64), "none"))
    # an arm over the run of N (arm B's anchor lies behind it)
    cases.append(("arm_over_N", turn_read(text, H, first_d + 500, first_d + N_RUN[1] + 5), "none"))
    cases.append(("arm_beside_N", turn_read(text, T, first_d + 500, first_d + N_RUN[1] + 1), None))
    # anchors in two sequences
    cases.append(("two_sequences", turn_read(text, H, 700, first_d + 480), "none"))
    cases.append(("two_sequences_T", turn_read(text, T, first_c + 100, first_d + 480), "none"))
    # same-strand records: a plain one counts for the span, one with three substitutions and a deletion leave no trace
    cases.append(("plain", text[first_d + 100:first_d + 100 + n], "span"))
    cases.append(("plain_craftA", a[900:900 + n], "span"))
    cases.append(("plain_over_turn", text[first_d + 50:first_d + 50 + n], "span"))
    sub3 = list(a[900:900 + n])
    for o in (40, 60, 100):
        sub3[o] = "ACGT"[("ACGT".index(sub3[o]) + 1) % 4]
    cases.append(("plain_mismatches", "".join(sub3), "none"))
    cases.append(("deletion", a[700:775] + a[1175:1250], "none"))
    out = []
    for label, read, expect in cases:
        assert set(read) <= set("ACGT"), label
        out.append((label, read, expect))
        out.append((label + "/rc", revcomp(read), expect))
    return out, text


# ---- a sample of random reads ------------------------------------------------------------------------------------------------------
def plant_palindromes(text: str, seed: int, n_sites: int = 12, lo: int = 500):
    """(the genome with n_sites pairs of reverse-complementary stretches of 1 to 8 bases written into it, the sites as (u, v, h))"""
    rng = random.Random(seed)
    t = list(text)
    sites = []
    span = (len(text) - 2 * lo) // (2 * n_sites)
    for i in range(n_sites):
        u, v, h = lo + (2 * i) * span, lo + (2 * i + 1) * span, rng.randrange(1, 9)
        t[u:u + h] = revcomp("".join(t[v - h + 1:v + 1]))
        sites.append((u, v, h))
    return "".join(t), sites


def sample_reads(text: str, sites, seed: int, n_reads: int = 2000, lengths=(64, 150), switch: float = 0.5, margin: int = 200):
    """Random reads of one sequence `text` (ACGT only between margin and its end less margin): a share `switch` of them turn -- half
    of those at a planted site (a random step into its shared stretch), the others at random pairs of cells, now and then a hairpin
    --, both kinds, each with 0 to 2 substitutions (a few with 4); the rest are plain reads, 0.5 % of their bases substituted.
    Half of all reads are reverse-complemented."""
    rng = random.Random(seed)
    reads = []
    for _ in range(n_reads):
        n = rng.randrange(lengths[0], lengths[1] + 1)
        if rng.random() < switch:
            kind = rng.choice((H, T))
            la = rng.randrange(25, n - 24)
            if rng.random() < 0.5:
                u, v, h = rng.choice(sites)
                t = rng.randrange(0, h + 1)
                x, y = (u - 1 + t, v - t) if kind == H else (u + t, v + 1 - t)
            elif rng.random() < 0.1:
                x = y = rng.randrange(margin + n, len(text) - margin - n)
            else:
                x, y = (rng.randrange(margin + n, len(text) - margin - n) for _ in range(2))
            subs = tuple(rng.sample(range(n), rng.choice((0, 0, 1, 2, 4))))
            r = turn_read(text, kind, x, y, la, n - la, subs)
        else:
            start = rng.randrange(margin, len(text) - margin - n)
            out = list(text[start:start + n])
            for o in range(n):
                if rng.random() < 0.005:
                    out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
            r = "".join(out)
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    return reads


FUZZ_SEED = 5


def fuzz_world(seed: int = FUZZ_SEED, n_reads: int = 2500):
    """([(name, letters)] of a random genome -- fuzzA of 8,000 letters with 24 planted turn sites and a run of N in its first cells,
    fuzzB of 900 --, reads of 64 to 150 bases of fuzzA, half of them strand switches)"""
    rng = random.Random(seed)
    a, sites = plant_palindromes(_rand(rng, 8000), seed + 1, n_sites=24, lo=500)
    a = a[:60] + "N" * 15 + a[75:]
    b = _rand(rng, 900)
    return [("fuzzA", a), ("fuzzB", b)], sample_reads(a, sites, seed + 2, n_reads=n_reads)
