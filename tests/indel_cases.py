"""Inputs of the indel tests (tests/test_indels_cpu.py, tests/test_gpu_indels.py): a crafted two-sequence genome with its crafted
records, and a sample of random reads of a genome with planted indels.  What the rule makes of them is indels_ref's business."""
from __future__ import annotations

import random

from tests import indels_ref

N_LEN = 150


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def crafted_genome(k: int):
    """(name, letters) of two sequences.  The first carries a homopolymer run [300, 312), a dinucleotide repeat [500, 520), k + 24
    bases at 600 repeated at 1100, and a stretch of N [1300, 1320); the second starts with G and k T's."""
    rng = random.Random(1000 + k)
    a = list(_rand(rng, 1500))
    a[299:313] = "C" + "A" * 12 + "G"
    a[499:521] = "G" + "CA" * 10 + "T"
    a[1100:1100 + k + 24] = a[600:600 + k + 24]
    a[1299:1321] = "G" + "N" * 20 + "G"   # (the index reads N as A: no C behind them, or A..AC would be the second sequence's first k-mer reversed)
    b = "G" + "T" * k + "C" + _rand(rng, 700)
    return [("craftA", "".join(a)), ("craftB some words", b)]


def mut_read(ref: str, start: int, n: int, dele=None, ins=None, subs=()):
    """n bases of `ref` from `start` on, with `dele` = (cell, D) left out and `ins` = (cell, S) put in front of a cell; then the
    read's offsets `subs` changed to another base."""
    out, i = [], start
    while len(out) < n:
        if dele and i == dele[0]:
            i += dele[1]
            dele = None
            continue
        if ins and i == ins[0]:
            out.extend(ins[1])
            ins = None
        out.append(ref[i])
        i += 1
    out = out[:n]
    for o in subs:
        out[o] = "ACGT"[("ACGT".index(out[o]) + 1) % 4]
    return "".join(out)


def _free_pos(ref, lo, d):
    """The first cell >= lo at which a deletion of d (or an insertion) cannot slide to the left."""
    p = lo
    while ref[p - 1] == ref[p + d - 1]:
        p += 1
    return p


def _ins_seq(rng, ref, pos, n):
    """n letters to insert in front of `pos` that cannot rotate to the left"""
    while True:
        s = _rand(rng, n)
        if s[-1] != ref[pos - 1]:
            return s


def crafted_cases(k: int):
    """[(label, read, expect)] on crafted_genome(k); every read is there along and against the reference (label + '/rc').
    expect: ('del', cell, D) / ('ins', cell, S) the haplotype the record supports (before normalisation), 'span', 'none', or
    None where nothing but the twins' agreement is asked."""
    (_, a), (_, b) = crafted_genome(k)
    first_b = len(a)
    rng = random.Random(77 + k)
    n = N_LEN
    cases = []
    p800 = _free_pos(a, 800, 1)
    for d in (1, 2, 32, 33):
        pos = _free_pos(a, 800, d)
        cases.append(("del%d" % d, mut_read(a, pos - 70, n, dele=(pos, d)), ("del", pos, d) if d <= 32 else "none"))
    for i in (1, 12, 32):
        s = _ins_seq(rng, a, p800, i)
        cases.append(("ins%d" % i, mut_read(a, p800 - 70, n, ins=(p800, s)), ("ins", p800, s)))
    # inside each repeat: anchors outside it, and the first anchor ending inside it
    cases.append(("homo_out", mut_read(a, 230, n, dele=(306, 2)), ("del", 306, 2)))
    cases.append(("homo_in", mut_read(a, 304 - k, n, dele=(306, 2)), ("del", 306, 2)))
    cases.append(("dinuc_out", mut_read(a, 430, n, ins=(510, "CA")), ("ins", 510, "CA")))
    cases.append(("dinuc_in", mut_read(a, 508 - k, n, ins=(510, "CA")), ("ins", 510, "CA")))
    # the breakpoint exactly at a + k and exactly at b
    pos = _free_pos(a, 850, 3)
    cases.append(("bp_at_a_plus_k", mut_read(a, pos - k, n, dele=(pos, 3)), ("del", pos, 3)))
    cases.append(("bp_at_b", mut_read(a, pos - (n - k), n, dele=(pos, 3)), ("del", pos, 3)))
    cases.append(("bp_in_last_k", mut_read(a, pos - (n - k + 5), n, dele=(pos, 3)), "none"))
    # substitutions in the first k-mers: the anchor is try 2, 3, 4; no try is left
    for t, subs in enumerate(((3,), (3, 10), (3, 10, 18), (3, 10, 18, 26)), 2):
        cases.append(("anchor_try%d" % t, mut_read(a, pos - 70, n, dele=(pos, 3), subs=subs), ("del4", pos, 3) if t < 5 else "none"))
    cases.append(("m_eq_M", mut_read(a, pos - 70, n, dele=(pos, 3), subs=(58, 62)), ("del", pos, 3)))
    cases.append(("m_eq_M_plus_1", mut_read(a, pos - 70, n, dele=(pos, 3), subs=(58, 62, 84)), "none"))
    cases.append(("n_2k_minus_1", a[700:700 + 2 * k - 1], "none"))
    cases.append(("n_2k", a[700:700 + 2 * k], "span"))
    cases.append(("n_splits", a[700:800] + "N" + a[801:900], "span"))
    cases.append(("on_duplicate", a[600:600 + n], "none"))
    cases.append(("beside_duplicate", a[596:596 + n], "span"))
    s = _ins_seq(rng, a, 1220, 10)
    cases.append(("into_N", mut_read(a, 1160, n, ins=(1220, s)), "none"))
    s = _ins_seq(rng, a, 1440, 10)
    cases.append(("over_end", mut_read(a, 1500 - (n - 10), n, ins=(1440, s)), "none"))
    cases.append(("across_sequences", a[-75:] + b[:75], "none"))
    cases.append(("second_cell", mut_read(b, 0, n, dele=(k, 1)), ("delB", first_b + 1, 1)))
    used = set()
    for j in range(2):
        s = _ins_seq(rng, a, p800, 3)
        while s in used:
            s = _ins_seq(rng, a, p800, 3)
        used.add(s)
        cases.append(("two_ins_%d" % j, mut_read(a, p800 - 60, n, ins=(p800, s)), ("ins", p800, s)))
    cases.append(("plain", a[900:900 + n], "span"))
    out = []
    for label, read, expect in cases:
        out.append((label, read, expect))
        out.append((label + "/rc", "".join(indels_ref._COMP.get(c, "N") for c in reversed(read)), expect))
    return out


PLANTED = [("del", 700, 6, 1.0), ("ins", 880, 9, 0.5), ("del", 1060, 9, 0.2), ("ins", 1240, 1, 0.05), ("del", 1420, 1, 0.05), ("ins", 1600, 3, 0.02)]
SAMPLE_SPAN = (500, 1800)          # the reads are drawn from these cells of the genome
SAMPLE_SEED = 1


def sample_reads(g: str, seed: int = SAMPLE_SEED, n_reads: int = 2000, length: int = N_LEN):
    """(reads, planted events as (kind, cell, D or S, frequency)): `n_reads` random reads of both strands from SAMPLE_SPAN of the
    genome, each planted indel present in a read with its frequency, 0.5 % of the bases substituted."""
    rng = random.Random(seed)
    planted = []
    for kind, lo, ln, af in PLANTED:
        pos = _free_pos(g, lo, ln if kind == "del" else 1)
        planted.append((kind, pos, ln if kind == "del" else _ins_seq(rng, g, pos, ln), af))
    reads = []
    for _ in range(n_reads):
        start = rng.randrange(SAMPLE_SPAN[0], SAMPLE_SPAN[1] - length)
        dels = {p: d for kind, p, d, af in planted if kind == "del" and rng.random() < af}
        inss = {p: s for kind, p, s, af in planted if kind == "ins" and rng.random() < af}
        out, i = [], start
        while len(out) < length:
            if i in dels:
                i += dels.pop(i)
                continue
            if i in inss:
                out.extend(inss.pop(i))
            out.append(g[i])
            i += 1
        out = out[:length]
        for o in range(length):
            if rng.random() < 0.005:
                out[o] = "ACGT"[("ACGT".index(out[o]) + 1 + rng.randrange(3)) % 4]
        r = "".join(out)
        reads.append(indels_ref.revcomp(r) if rng.random() < 0.5 else r)
    return reads, planted


def haplotype(text: str, kind: int, cell: int, length: int, s: str) -> str:
    """The genome with one event applied"""
    return text[:cell] + s + text[cell + (length if kind == indels_ref.DEL else 0):]
