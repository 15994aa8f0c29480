"""The rule of `bronko call --consensus-indels`, restated in plain Python (include/bronko_hip.h bk_sample_consensus_indels, DESIGN.md
section CI): which of a sample's indel events are accepted at the consensus thresholds, which of those are applied, what the applied
ones make of the consensus letters, and the two files the writers make.

Written from the rule and not from the C++ or the kernels -- Python ints, sorted(), one float product --: the host twin
(bh_consensus_indels) and the engine (bk_consensus_indels.hip) are held against it.  Cells are the positions of all sequences of the
genome file, concatenated, as in tests/indels_ref.py, whose Genome and event keys are used here."""
from __future__ import annotations

from tests.indels_ref import DEL, INS, af_text, seq_code

TALLIES = ("candidates", "accepted", "applied", "contested", "deletions", "insertions", "deleted_bases", "inserted_bases", "frameshifts")
PAIRS = ((1, 0.0), (10, 0.5), (10, 0.25), (1, 1.0))      # the (D, F) pairs the tests run at


def events_of(res) -> list[tuple]:
    """An indels_ref.Result as this module's events: [(cell, kind, length, S, s)]"""
    return [(cell, kind, length, S, fwd + rev) for (cell, kind, length, S), (fwd, rev) in res.events.items()]


def is_accepted(s: int, r: int, D: int, F: float) -> bool:
    n = s + r
    return n >= D and float(s) >= F * float(n)


def occupied(cell: int, kind: int, length: int) -> range:
    """The boundaries an event occupies; boundary b lies in front of cell b."""
    return range(cell, cell + length + 1) if kind == DEL else range(cell, cell + 1)


def resolve(events, span_sums, D: int, F: float):
    """events [(cell, kind, length, S, s)], every candidate; span_sums the prefix-summed span array.  Returns (rows, tallies): rows
    [(cell, kind, length, S, s, r, applied)] of the accepted events sorted by (cell, kind, length, seq)."""
    acc = [(cell, kind, length, S, s, span_sums[cell]) for cell, kind, length, S, s in events if is_accepted(s, span_sums[cell], D, F)]
    acc = sorted(acc, key=lambda e: (e[0], e[1], e[2], seq_code(e[3])))
    rows = []
    for i, (cell, kind, length, S, s, r) in enumerate(acc):
        mine = occupied(cell, kind, length)
        applied = True
        for j, o in enumerate(acc):
            if j != i and any(b in mine for b in occupied(o[0], o[1], o[2])) and not s > o[4]:
                applied = False
        rows.append((cell, kind, length, S, s, r, applied))
    done = [r for r in rows if r[6]]
    t = dict(candidates=len(events), accepted=len(rows), applied=len(done), contested=len(rows) - len(done),
             deletions=sum(1 for r in done if r[1] == DEL), insertions=sum(1 for r in done if r[1] == INS),
             deleted_bases=sum(r[2] for r in done if r[1] == DEL), inserted_bases=sum(r[2] for r in done if r[1] == INS),
             frameshifts=sum(1 for r in done if r[2] % 3 != 0))
    return rows, t


def edit_letters(letters: bytes, rows, cell0: int = 0) -> bytes:
    """The consensus letters of the genome file (its first cell: cell0) with '-' at the cells of the applied deletions"""
    out = bytearray(letters)
    for cell, kind, length, S, s, r, applied in rows:
        if applied and kind == DEL:
            for c in range(cell, cell + length):
                out[c - cell0] = ord("-")
    return bytes(out)


def abi_rows(rows) -> list[tuple]:
    """rows as the engine and the twin give them: (cell, len, support, ref_span, seq, applied); len > 0 a deletion, < 0 an insertion"""
    return [(cell, length if kind == DEL else -length, s, r, seq_code(S), 1 if applied else 0) for cell, kind, length, S, s, r, applied in rows]


def _edited(g, q: int, letters: bytes, rows):
    """Sequence q after the edit: [(letter, the cell it came from or None for an inserted one)]"""
    put = {cell: S for cell, kind, length, S, s, r, applied in rows if applied and kind == INS}
    out = []
    for cell in range(g.first[q], g.first[q] + len(g.seqs[q])):
        for c in put.get(cell, ""):
            out.append((c, None))
        if letters[cell:cell + 1] != b"-":
            out.append((chr(letters[cell]), cell))
    return out


def fasta_text(g, stem: str, letters: bytes, rows) -> str:
    """OUT/<stem>.consensus.fa of the edited letters (those of edit_letters): lines of 60 after the edit"""
    out = []
    for q, name in enumerate(g.names):
        out.append(">%s|%s" % (stem, name))
        text = "".join(c for c, _ in _edited(g, q, letters, rows))
        out.extend(text[i:i + 60] for i in range(0, len(text), 60))
    return "".join(line + "\n" for line in out)


def tsv_text(g, letters: bytes, rows, D: int, F: float) -> str:
    """OUT/<stem>.consensus_indels.tsv: a line per accepted event; cons_pos, the 1-based place in the edited sequence of the base
    in front of an applied event, is looked up in the edited sequence itself"""
    out = ["##consensus_min_depth=%d" % D, "##consensus_min_freq=%g" % F,
           "\t".join(["chrom", "pos", "type", "len", "seq", "support", "ref_span", "af", "status", "cons_pos"])]
    for cell, kind, length, S, s, r, applied in sorted(rows, key=lambda e: (e[0], e[1], e[2], seq_code(e[3]))):
        q = g.seq_of(cell)
        cons_pos = "."
        if applied:
            origins = [o for _, o in _edited(g, q, letters, rows)]
            cons_pos = str(origins.index(cell - 1) + 1)
        out.append("\t".join([g.names[q], str(cell - g.first[q]), "DEL" if kind == DEL else "INS", str(length), S if kind == INS else ".", str(s), str(r),
                              af_text(s, r), "applied" if applied else "contested", cons_pos]))
    return "".join(line + "\n" for line in out)
