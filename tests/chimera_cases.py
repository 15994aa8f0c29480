"""Inputs of the chimera tests (tests/test_chimeras_cpu.py, tests/test_gpu_chimeras.py): crafted records on the duplication tests'
crafted genome with two more sequences, and samples of random reads that join two sequences.  What the rule makes of them is
chimeras_ref's business."""
from __future__ import annotations

import random

from tests import duplication_cases
from tests.chimeras_ref import L, R, revcomp
from tests.indel_cases import _rand

N_LEN = 150
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
E_N_RUN = (900, 920)    # craftE's run of N
EDGE = 4                # bases of the stretches that craftF shares with craftE's first cells, last cells and the cells behind its run of N


def _other(c: str, *avoid: str) -> str:
    return next(x for x in "ACGT" if x != c and x not in avoid)


def along_sites(k: int):
    """label -> (u, v, h), offsets in craftE and craftF: F[v, v + h) are the letters of E[u, u + h), and the letters on either side
    differ.  A junction of two arms along the reference (or both against it) that leaves E at u - 1 + t and goes on in F at v + t, or
    leaves F at v - 1 + t and goes on in E at u + t, is the same for t in [0, h]."""
    return {"one": (150, 120, 1), "six": (250, 220, 6), "k_minus_1": (350, 320, k - 1)}


def turned_sites(k: int):
    """label -> (u, v, h): F[v - h + 1, v + 1) is the reverse complement of E[u, u + h), and the letters on either side are not.  A
    junction that runs up E to u - 1 + t and comes down F from v - t (sides L, L), or runs down E to u + h - t and goes up F from
    v - h + 1 + t (sides R, R), is the same for t in [0, h]."""
    return {"one": (500, 470, 1), "six": (600, 580, 6), "k_minus_1": (700, 690, k - 1)}


def edge_sites():
    """label -> (cell offset in craftE, offset in craftF) of the EDGE bases that craftF holds of craftE's first cells, of its last
    cells and of the cells behind its run of N; the letter in front of (behind) the copy in craftF is the one that lies in front of
    (behind) the stretch in the index, so that cell arithmetic alone would slide on."""
    return {"first": (0, 800), "last": (-EDGE, 900), "n_run": (E_N_RUN[1], 1000)}


def crafted_genome(k: int):
    """duplication_cases.crafted_genome(k) -- craftA to craftD, their cells where they are -- and behind them craftE (random letters
    with the run E_N_RUN) and craftF (random letters with the copies of along_sites, the reverse-complemented copies of turned_sites
    and the three stretches of edge_sites)."""
    base = duplication_cases.crafted_genome(k)
    rng = random.Random(4000 + k)
    e, f = list(_rand(rng, 1200)), list(_rand(rng, 1200))
    e[E_N_RUN[0] - 1:E_N_RUN[1] + 1] = "G" + "N" * (E_N_RUN[1] - E_N_RUN[0]) + "G"
    for (u, v, h) in along_sites(k).values():
        f[v:v + h] = e[u:u + h]
        f[v - 1], f[v + h] = _other(e[u - 1]), _other(e[u + h])
    for (u, v, h) in turned_sites(k).values():
        f[v - h + 1:v + 1] = revcomp("".join(e[u:u + h]))
        f[v + 1], f[v - h] = _other(_COMP[e[u - 1]]), _other(_COMP[e[u + h]])
    d_last = base[-1][1][-1]
    sites = edge_sites()
    v = sites["first"][1]                            # E's first cells: in front of them lies craftD's last letter
    f[v:v + EDGE] = e[:EDGE]
    f[v - 1], f[v + EDGE] = d_last, _other(e[EDGE])
    v = sites["last"][1]                             # E's last cells: behind them lies craftF's first letter
    f[v:v + EDGE] = e[len(e) - EDGE:]
    f[v - 1], f[v + EDGE] = _other(e[len(e) - EDGE - 1]), f[0]
    v = sites["n_run"][1]                            # behind the run of N, whose cells the engine's reference holds as A
    f[v:v + EDGE] = e[E_N_RUN[1]:E_N_RUN[1] + EDGE]
    f[v - 1], f[v + EDGE] = "A", _other(e[E_N_RUN[1] + EDGE])
    return base + [("craftE", "".join(e)), ("craftF", "".join(f))]


def arm_text(ref: str, cell: int, side: int, length: int, first: bool) -> str:
    """The bases a read shows of an arm of `length` cells that ends (arm A, `first`) or begins (arm B) at `cell`: side L holds the cell
    and the cells below it, side R the cell and the cells above it.  Arm A with side L and arm B with side R run along the reference;
    the other two run against it.  Letters that are not ACGT read as A."""
    if side == L:
        assert cell - length + 1 >= 0
        s = ref[cell - length + 1:cell + 1].replace("N", "A")
        return s if first else revcomp(s)
    s = ref[cell:cell + length].replace("N", "A")
    assert len(s) == length
    return revcomp(s) if first else s


def chimera_read(ref: str, x: int, side_x: int, y: int, side_y: int, la: int = N_LEN // 2, lb: int = N_LEN - N_LEN // 2, subs=()) -> str:
    """A read that leaves the reference at cell x and goes on at cell y: la bases of arm A that end at the base of x, lb bases of arm
    B that begin at the base of y; the offsets `subs` changed to another base."""
    out = list(arm_text(ref, x, side_x, la, True) + arm_text(ref, y, side_y, lb, False))
    for o in subs:
        out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
    return "".join(out)


def _shown(ref: str, cell: int, along: bool) -> str:
    return ref[cell] if along else _COMP.get(ref[cell], "?")


def slides(ref: str, x: int, side_x: int, y: int, side_y: int) -> bool:
    """Whether the pair of cells could move one base either way by the letters alone (no sequence border, no N is looked at)"""
    da, db = (1 if side_x == L else -1), (1 if side_y == R else -1)
    up = _shown(ref, x + da, da > 0) == _shown(ref, y, db > 0)
    down = _shown(ref, x, da > 0) == _shown(ref, y - db, db > 0)
    return up or down


def free_pair(ref: str, x: int, y: int, sides=((L, R), (L, L), (R, R), (R, L))):
    """The first pair (x' >= x, y <= y' < y + 100) that cannot slide either way in any of the orientations `sides`"""
    while True:
        for yy in range(y, y + 100):
            if not any(slides(ref, x, sx, yy, sy) for sx, sy in sides):
                return x, yy
        x += 1


def event(x: int, side_x: int, y: int, side_y: int):
    return ("ch", x, side_x, y, side_y) if x < y else ("ch", y, side_y, x, side_x)


ORIENTATIONS = (("LR", L, R), ("LL", L, L), ("RR", R, R), ("RL", R, L))   # (arm A's side, arm B's side): along/along, along/against, against/along, against/against


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(k); every read is there as it is and reverse-complemented (label + '/rc').
    expect, at 2 mismatches: ('ch', lo, side_lo, hi, side_hi) the event the record supports, 'span', 'discordant', 'none' for a
    record that leaves no tally behind `crossed` or `same_strand`, 'nothing' for one that leaves none behind `records`."""
    seqs = crafted_genome(k)
    text = "".join(s for _, s in seqs)
    first = [0]
    for _, s in seqs:
        first.append(first[-1] + len(s))
    a = seqs[0][1]
    fa, fb, fc, fd, fe, ff, end = first
    n, half = N_LEN, N_LEN // 2
    cases = []

    x, y = free_pair(text, fe + 450, ff + 150)       # arm A in craftE, arm B in craftF: all four side combinations at the same two cells
    xr, yr = free_pair(text, ff + 560, fe + 300)     # arm A in craftF, arm B in craftE
    for name, sx, sy in ORIENTATIONS:
        cases.append((name + "_e_then_f", chimera_read(text, x, sx, y, sy), event(x, sx, y, sy)))
        cases.append((name + "_f_then_e", chimera_read(text, xr, sx, yr, sy), event(xr, sx, yr, sy)))
        cases.append((name + "_bp_at_f_plus_k", chimera_read(text, x, sx, y, sy, k, n - k), event(x, sx, y, sy)))
        cases.append((name + "_bp_at_g", chimera_read(text, x, sx, y, sy, n - k, k), event(x, sx, y, sy)))
        cases.append((name + "_bp_in_last_k", chimera_read(text, x, sx, y, sy, n - k + 5, k - 5), None))
        cases.append((name + "_bp_in_first_k", chimera_read(text, x, sx, y, sy, k - 5, n - k + 5), None))
        cases.append((name + "_n_2k", chimera_read(text, x, sx, y, sy, k, k), event(x, sx, y, sy)))
        cases.append((name + "_n_2k_minus_1", chimera_read(text, x, sx, y, sy, k, k - 1), "nothing"))
        cases.append((name + "_n_64", chimera_read(text, x, sx, y, sy, 32, 32), event(x, sx, y, sy)))
        cases.append((name + "_sub_at_p_minus_1", chimera_read(text, x, sx, y, sy, subs=(half - 1,)), None))
        cases.append((name + "_sub_at_p", chimera_read(text, x, sx, y, sy, subs=(half,)), None))
        cases.append((name + "_m_eq_M", chimera_read(text, x, sx, y, sy, subs=(40, 100)), event(x, sx, y, sy)))
        cases.append((name + "_m_eq_M_plus_1", chimera_read(text, x, sx, y, sy, subs=(40, 60, 100)), "discordant"))
        cases.append((name + "_anchor_try2_front", chimera_read(text, x, sx, y, sy, subs=(3,)), event(x, sx, y, sy)))
        cases.append((name + "_anchor_try3_front", chimera_read(text, x, sx, y, sy, subs=(3, 10)), event(x, sx, y, sy)))
        cases.append((name + "_anchor_try2_back", chimera_read(text, x, sx, y, sy, subs=(n - 4,)), event(x, sx, y, sy)))
        cases.append((name + "_anchor_try3_back", chimera_read(text, x, sx, y, sy, subs=(n - 4, n - 11)), event(x, sx, y, sy)))
    # homology of 1, 6 and k - 1 bases: the record breaks in the middle of the shared stretch, the event is the run's lower end in
    # craftE.  Two arms on one strand share along_sites' stretches, two arms on two strands turned_sites'.
    for label, (u, v, h) in along_sites(k).items():
        t = (h + 1) // 2
        cases.append(("LR_homology_" + label, chimera_read(text, fe + u - 1 + t, L, ff + v + t, R), ("ch", fe + u - 1, L, ff + v, R)))
        cases.append(("LR_homology_f_then_e_" + label, chimera_read(text, ff + v - 1 + t, L, fe + u + t, R), ("ch", fe + u, R, ff + v - 1, L)))
        cases.append(("RL_homology_" + label, chimera_read(text, fe + u + t, R, ff + v - 1 + t, L), ("ch", fe + u, R, ff + v - 1, L)))
    for label, (u, v, h) in turned_sites(k).items():
        t = (h + 1) // 2
        cases.append(("LL_homology_" + label, chimera_read(text, fe + u - 1 + t, L, ff + v - t, L), ("ch", fe + u - 1, L, ff + v, L)))
        cases.append(("RR_homology_" + label, chimera_read(text, fe + u + h - t, R, ff + v - h + 1 + t, R), ("ch", fe + u, R, ff + v + 1, R)))
    # a slide that a sequence's first cell, its last cell and the run of N stop, where the letters would let it go on.  (Arm A's cells
    # are those of the offsets in front of the back anchor, arm B's those behind the front anchor: an arm that ends two cells from a
    # border is placed where the anchor beyond the breakpoint ends two bases from it.)
    sites = edge_sites()
    v = ff + sites["first"][1]                       # arm B begins in craftE's first cells: no pair below E's first cell
    cases.append(("slide_stops_at_first_cell", chimera_read(text, v + 1, L, fe + 2, R, k + 2, n - k - 2), ("ch", fe, R, v - 1, L)))
    v = ff + sites["last"][1]                        # arm A ends in craftE's last cells: the run's low end is where the letters end it
    cases.append(("slide_stops_at_last_cell", chimera_read(text, ff - 3, L, v + 2, R, n - k - 2, k + 2), ("ch", ff - EDGE - 1, L, v, R)))
    v = ff + sites["n_run"][1]                       # arm B begins behind the run of N
    cases.append(("slide_stops_at_n_run", chimera_read(text, v + 1, L, fe + E_N_RUN[1] + 2, R, k + 2, n - k - 2), ("ch", fe + E_N_RUN[1], R, v - 1, L)))
    # an arm that ends at its sequence's last cell joined to an arm that begins at another's first: both anchors end at the
    # breakpoint, f + k = g.  Then the two sequences neighbours in the index, on one strand: delta = 0 in cell arithmetic.
    cases.append(("last_of_d_first_of_f", text[fe - k:fe] + text[ff:ff + k], ("ch", fe - 1, L, ff, R)))
    cases.append(("last_of_e_first_of_f", text[ff - k:ff + k], ("ch", ff - 1, L, ff, R)))
    cases.append(("last_of_d_first_of_e", text[fe - k:fe + k], ("ch", fe - 1, L, fe, R)))
    cases.append(("last_of_a_first_of_b_try2", chimera_read(text, fb - 1, L, fb, R, k + 8, k, subs=(3,)), ("ch", fb - 1, L, fb, R)))
    cases.append(("first_of_f_last_of_e_turned", chimera_read(text, ff, R, ff - 1, L, k, k), ("ch", ff - 1, L, ff, R)))
    cases.append(("last_of_e_first_of_f_one_base_more", text[ff - k - 1:ff + k], "none"))   # arm A's cells run into craftF
    # an arm that would walk out of its sequence into the neighbour's letters: ten bases of craftD's end in front of craftE's first
    # cells (the front anchor is the third try, inside craftE); ten of craftF's first behind craftE's last
    cases.append(("arm_a_leaves_sequence", text[fe - 10:fe + 65] + text[ff + 500:ff + 575], "none"))
    cases.append(("arm_b_leaves_sequence", text[fc + 100:fc + 175] + text[ff - 65:ff + 10], "none"))
    # a run of N under an arm (the anchors lie clear of it)
    cases.append(("arm_a_over_N", chimera_read(text, fe + E_N_RUN[1] + 10, L, ff + 500, R), "none"))
    cases.append(("arm_b_over_N", chimera_read(text, ff + 500, L, fe + E_N_RUN[0] - 10, R), "none"))
    xn, yn = free_pair(text, ff + 500, fe + E_N_RUN[1] + 1, ((L, R),))
    cases.append(("arm_b_beside_N", chimera_read(text, xn, L, yn, R, k, n - k), event(xn, L, yn, R)))
    # records of one sequence: a deletion and a duplication are same_strand and nothing else, a copy-back leaves no tally at all
    cases.append(("deletion", a[700:775] + a[1175:1250], "none"))
    cases.append(("duplication", duplication_cases.dup_read(a, duplication_cases.free_pos(a, 1200, 200), 200), "none"))
    cases.append(("copyback", chimera_read(text, fe + 450, L, fe + 200, L), "nothing"))
    cases.append(("copyback_T", chimera_read(text, fe + 450, R, fe + 200, R), "nothing"))
    # plain records count for the span, one with three substitutions leaves no trace; foreign reads
    cases.append(("plain_e", text[fe + 100:fe + 100 + n], "span"))
    cases.append(("plain_f", text[ff + 80:ff + 80 + n], "span"))
    cases.append(("plain_over_junction_cell", text[x - 50:x + 100], "span"))
    cases.append(("plain_last_of_f", text[end - n:end], "span"))
    sub3 = list(a[900:900 + n])
    for o in (40, 60, 100):
        sub3[o] = "ACGT"[("ACGT".index(sub3[o]) + 1) % 4]
    cases.append(("plain_mismatches", "".join(sub3), "none"))
    rng = random.Random(91)
    cases.append(("foreign", _rand(rng, n), "nothing"))
    cases.append(("foreign_back", text[fe + 100:fe + 100 + half] + _rand(rng, n - half), "nothing"))
    out = []
    for label, read, expect in cases:
        assert set(read) <= set("ACGT"), label
        out.append((label, read, expect))
        out.append((label + "/rc", revcomp(read), expect))
    return out, text


# ---- a sample of random reads ------------------------------------------------------------------------------------------------------
FUZZ_SEED = 7


def fuzz_genome(seed: int):
    """[(name, letters)] of three to five sequences of 1,500 to 3,000 random letters: stretches of 1 to 8 bases of each copied into
    the next one, as they are and reverse-complemented (the sites of fuzz_reads), a repeat of 40 bases shared by two sequences as it
    is and one reverse-complemented (no anchors there), a run of N; and the sites as (sequence, offset, sequence, offset, h, turned)."""
    rng = random.Random(seed)
    seqs = [list(_rand(rng, rng.randrange(1500, 3001))) for _ in range(rng.randrange(3, 6))]
    sites = []
    for s in range(len(seqs)):
        q = (s + 1) % len(seqs)
        for i in range(8):
            h, turned = rng.randrange(1, 9), i % 2 == 1
            u, v = 300 + 100 * i, 350 + 100 * i
            piece = "".join(seqs[s][u:u + h])
            seqs[q][v:v + h] = revcomp(piece) if turned else piece
            sites.append((s, u, q, v, h, turned))
    seqs[1][1200:1240] = seqs[0][1250:1290]
    seqs[2][1300:1340] = revcomp("".join(seqs[0][1350:1390]))
    at = 315 + 100 * rng.randrange(8) + rng.randrange(15)          # (between two sites)
    seqs[0][at:at + 15] = "N" * 15
    return [("fuzz%d" % i, "".join(s)) for i, s in enumerate(seqs)], sites


def fuzz_reads(seqs, sites, seed: int, n_reads: int, lengths=(64, 150), crossed: float = 0.6, margin: int = 250):
    """Random reads: a share `crossed` of them join two sequences -- a third of those at a planted site (a random step into its
    shared stretch), the others at random cells --, the four side combinations equally often, with 0 to 2 substitutions (a few with
    4); of the rest most are plain reads with 0.5 % of their bases substituted, some carry a deletion, some turn inside one sequence.
    Half of all reads are reverse-complemented."""
    rng = random.Random(seed)
    text = "".join(s for _, s in seqs)
    first = [0]
    for _, s in seqs:
        first.append(first[-1] + len(s))
    reads = []

    def cell_in(s, n):
        return rng.randrange(first[s] + margin + n, first[s + 1] - margin - n)

    for _ in range(n_reads):
        n = rng.randrange(lengths[0], lengths[1] + 1)
        u = rng.random()
        if u < crossed:
            la = rng.randrange(25, n - 24)
            if rng.random() < 0.33:
                s, a, q, b, h, turned = rng.choice(sites)
                t = rng.randrange(0, h + 1)
                if not turned:
                    x, sx, y, sy = rng.choice(((first[s] + a - 1 + t, L, first[q] + b + t, R), (first[s] + a + t, R, first[q] + b - 1 + t, L)))
                else:
                    x, sx, y, sy = rng.choice(((first[s] + a - 1 + t, L, first[q] + b + h - 1 - t, L), (first[s] + a + h - t, R, first[q] + b + t, R)))
                if rng.random() < 0.5:                             # the same junction met from its other cell
                    x, sx, y, sy = y, sy, x, sx
            else:
                s, q = rng.sample(range(len(seqs)), 2)
                x, y = cell_in(s, n), cell_in(q, n)
                sx, sy = rng.choice((L, R)), rng.choice((L, R))
            subs = tuple(rng.sample(range(n), rng.choice((0, 0, 1, 2, 4))))
            r = chimera_read(text, x, sx, y, sy, la, n - la, subs)
        elif u < crossed + 0.05:                                   # a turn inside one sequence
            s = rng.randrange(len(seqs))
            side = rng.choice((L, R))
            r = chimera_read(text, cell_in(s, n), side, cell_in(s, n), side, n // 2, n - n // 2)
        else:
            s = rng.randrange(len(seqs))
            start = rng.randrange(first[s] + margin, first[s + 1] - margin - n - 40)
            out = list(text[start:start + n])
            if u < crossed + 0.10:                                 # a deletion of 5 to 40 bases
                cut = rng.randrange(5, 41)
                out = list(text[start:start + n // 2] + text[start + n // 2 + cut:start + n + cut])
            for o in range(n):
                if rng.random() < 0.005 and out[o] != "N":
                    out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
            r = "".join(out).replace("N", "A")
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    return reads


def fuzz_world(seed: int = FUZZ_SEED, n_reads: int = 2500):
    """([(name, letters)] of fuzz_genome(seed), reads of 64 to 150 bases, six in ten of them junctions between two sequences)"""
    seqs, sites = fuzz_genome(seed)
    return seqs, fuzz_reads(seqs, sites, seed + 2, n_reads)
