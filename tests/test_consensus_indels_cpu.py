"""`bronko call --consensus-indels` without a GPU: the host twin (bronko_amd/host/consensus_indels.cpp through bh_consensus_indels)
against the Python restatement of the rule (tests/consensus_indels_ref.py) on crafted event lists over indel_cases.crafted_genome(21)
-- every accepted event with its status, every tally, the edited letters --, the two writers byte for byte, and the argument errors
of `bronko call`.  No reads: an event is (cell, kind, length, S, s, r), the reads that support it and those that span its cell."""
import os
import random
import subprocess

import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import consensus_indels_ref as ref
from tests import indel_cases, indels_ref
from tests.indels_ref import DEL, INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
K = 21


class World:
    def __init__(self):
        seqs = indel_cases.crafted_genome(K)
        self.ix = HostIndex.build_mem(K, [("crafted", [(name, s.encode()) for name, s in seqs])])
        self.g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], K)
        self.letters = self.g.text.encode()                          # (any letters do: the reference's own, its N included)
        self.first_b = self.g.first[1]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ix.close()


def _both(w, events, D, F):
    """The twin and the restatement on the same events [(cell, kind, length, S, s, r)] (one r per cell); asserts that they agree in
    rows, tallies and letters and returns the restatement's (rows, tallies, edited letters)."""
    span = [0] * (w.g.cells + 2)
    for cell, kind, length, S, s, r in events:
        assert span[cell] in (0, r)
        span[cell] = r
    rows, tallies = ref.resolve([e[:5] for e in events], span, D, F)
    edited = ref.edit_letters(w.letters, rows)
    table = [(cell, length if kind == DEL else -length, s // 2, s - s // 2, r, indels_ref.seq_code(S)) for cell, kind, length, S, s, r in events]
    got_rows, got_tallies, got_letters = hostlib.consensus_indels(w.ix, 0, table, span[:w.g.cells], w.letters, D, F)
    assert got_rows == ref.abi_rows(rows), (D, F, [r for r in got_rows if r not in ref.abi_rows(rows)][:3], [r for r in ref.abi_rows(rows) if r not in got_rows][:3])
    assert got_tallies == tallies, (D, F)
    assert got_letters == edited, (D, F)
    assert tallies["accepted"] == tallies["applied"] + tallies["contested"] and tallies["applied"] == tallies["deletions"] + tallies["insertions"]
    assert edited.count(b"-") - w.letters.count(b"-") == tallies["deleted_bases"]
    return rows, tallies, edited


def _status(rows):
    """{(cell, kind, length, S): applied}"""
    return {r[:4]: r[6] for r in rows}


# ---- conflicts --------------------------------------------------------------------------------------------------------------------
def test_overlapping_deletions(world):
    a, b = (100, DEL, 5, ""), (103, DEL, 4, "")
    st = _status(_both(world, [a + (20, 0), b + (8, 0)], 1, 0.0)[0])
    assert st == {a: True, b: False}                                 # the higher is applied, the lower contested
    st = _status(_both(world, [a + (8, 0), b + (20, 0)], 1, 0.0)[0])
    assert st == {a: False, b: True}
    rows, t, edited = _both(world, [a + (12, 0), b + (12, 0)], 1, 0.0)
    assert _status(rows) == {a: False, b: False} and t["contested"] == 2 and edited == world.letters   # equal support contests both


def test_adjacent_deletions_collide(world):
    a, b = (400, DEL, 3, ""), (403, DEL, 2, "")                      # they share the boundary 403
    assert _status(_both(world, [a + (9, 1), b + (7, 2)], 1, 0.0)[0]) == {a: True, b: False}
    c = (404, DEL, 2, "")                                            # one cell further: no boundary in common
    assert _status(_both(world, [a + (9, 1), c + (7, 2)], 1, 0.0)[0]) == {a: True, c: True}


def test_insertions_at_the_edges_of_a_deletion(world):
    d = (200, DEL, 4, "")                                            # boundaries 200 .. 204
    for cell, collide in ((200, True), (204, True), (202, True), (205, False), (199, False)):
        i = (cell, INS, 2, "AC")
        st = _status(_both(world, [d + (15, 3), i + (10, 3)], 1, 0.0)[0])
        assert st == {d: True, i: not collide}, cell
        st = _status(_both(world, [d + (10, 3), i + (15, 3)], 1, 0.0)[0])
        assert st == {d: not collide, i: True}, cell
        st = _status(_both(world, [d + (10, 3), i + (10, 3)], 1, 0.0)[0])
        assert st == {d: not collide, i: not collide}, cell


def test_a_chain_has_one_round(world):
    a, b, c = (300, DEL, 5, ""), (305, DEL, 5, ""), (310, DEL, 3, "")   # a and b share 305, b and c share 310; a and c nothing
    rows, t, _ = _both(world, [a + (30, 0), b + (20, 0), c + (10, 0)], 1, 0.0)
    assert _status(rows) == {a: True, b: False, c: False}            # c lost to b and stays contested though b lost too
    assert (t["applied"], t["contested"], t["deleted_bases"]) == (1, 2, 5)


def test_two_insertions_at_one_cell(world):
    x, y = (600, INS, 3, "ACG"), (600, INS, 3, "ACT")
    assert _status(_both(world, [x + (9, 4), y + (5, 4)], 1, 0.0)[0]) == {x: True, y: False}
    assert _status(_both(world, [x + (5, 4), y + (5, 4)], 1, 0.0)[0]) == {x: False, y: False}
    z = (600, INS, 1, "G")                                           # ... and of different lengths
    assert _status(_both(world, [x + (5, 4), y + (4, 4), z + (6, 4)], 1, 0.0)[0]) == {x: False, y: False, z: True}


def test_a_rejected_event_contests_nothing(world):
    a, b = (100, DEL, 5, ""), (103, DEL, 4, "")
    rows, t, _ = _both(world, [a + (12, 0), b + (20, 30)], 10, 0.5)   # b has more reads but is below F: it is no accepted event
    assert _status(rows) == {a: True} and (t["candidates"], t["accepted"]) == (2, 1)
    rows, t, _ = _both(world, [a + (12, 0), b + (20, 30)], 10, 0.25)  # ... and at a lower F it is one
    assert _status(rows) == {a: False, b: True}


# ---- thresholds -------------------------------------------------------------------------------------------------------------------
def test_thresholds(world):
    e = (700, DEL, 2, "")
    assert _both(world, [e + (5, 4)], 10, 0.5)[1]["accepted"] == 0   # n = D - 1
    assert _both(world, [e + (5, 5)], 10, 0.5)[1]["accepted"] == 1   # n = D, s = 5, r = 5 at F = 0.5
    assert _both(world, [e + (4, 5)], 1, 0.5)[1]["accepted"] == 0    # s = 4, r = 5 at F = 0.5
    assert _both(world, [e + (4, 5)], 9, 0.0)[1]["accepted"] == 1    # F = 0 accepts everything with n >= D
    assert _both(world, [e + (1, 500)], 1, 0.0)[1]["accepted"] == 1
    assert _both(world, [e + (1, 8)], 10, 0.0)[1]["accepted"] == 0
    assert _both(world, [e + (50, 1)], 1, 1.0)[1]["accepted"] == 0   # F = 1 needs r = 0
    assert _both(world, [e + (50, 0)], 1, 1.0)[1]["accepted"] == 1
    assert _both(world, [e + (1, 2)], 1, 1 / 3)[1]["accepted"] == (1 if 1.0 >= (1 / 3) * 3.0 else 0)   # the one float product decides


# ---- sizes and tallies ------------------------------------------------------------------------------------------------------------
def test_length_32_and_the_tallies(world):
    s32 = "ACGT" * 7 + "TTGT"
    events = [(150, DEL, 32, "", 9, 1), (250, INS, 32, s32, 8, 2), (350, DEL, 3, "", 7, 0), (450, INS, 6, "ACGTAC", 7, 0), (550, INS, 1, "T", 7, 0),
              (world.first_b + 40, DEL, 31, "", 5, 0), (650, DEL, 2, "", 1, 30)]
    rows, t, edited = _both(world, events, 5, 0.5)
    assert t == dict(candidates=7, accepted=6, applied=6, contested=0, deletions=3, insertions=3, deleted_bases=66, inserted_bases=39, frameshifts=4)
    assert edited[150:182] == b"-" * 32 and edited[149:150] != b"-" and edited[182:183] != b"-"
    assert indels_ref.seq_code(s32) >= 1 << 63                       # all 64 bits of seq are in use


# ---- random sets ------------------------------------------------------------------------------------------------------------------
def _random_events(rng, w):
    lo = rng.choice([60, 700, w.first_b + 30])
    span_of = {}
    events = {}
    for _ in range(rng.randrange(2, 40)):
        cell = lo + rng.randrange(0, rng.choice([12, 60, 200]))
        kind = rng.choice([DEL, INS])
        length = rng.choice([1, 1, 2, 3, 3, 4, 6, 9, 17, 32])
        S = "".join(rng.choice("ACGT") for _ in range(length)) if kind == INS else ""
        r = span_of.setdefault(cell, rng.choice([0, 0, 1, 5, 10, 40]))
        events[(cell, kind, length, S)] = (rng.choice([1, 2, 5, 5, 10, 10, 11, 30]), r)
    return [key + val for key, val in events.items()]


def test_random_sets(world):
    rng = random.Random(20)
    seen = dict(applied=0, contested=0, rejected=0)
    for _ in range(200):
        events = _random_events(rng, world)
        for D, F in ref.PAIRS:
            rows, t, _ = _both(world, events, D, F)
            seen["applied"] += t["applied"]
            seen["contested"] += t["contested"]
            seen["rejected"] += t["candidates"] - t["accepted"]
    assert min(seen.values()) > 500, seen


# ---- the writers ------------------------------------------------------------------------------------------------------------------
def _files(w, tmp_path, events, D, F, stem="s1"):
    rows, t, edited = _both(w, events, D, F)
    fa, tsv = str(tmp_path / "x.consensus.fa"), str(tmp_path / "x.consensus_indels.tsv")
    hostlib.write_consensus_indels_fasta(fa, stem, w.ix, 0, edited, ref.abi_rows(rows))
    hostlib.write_consensus_indels_tsv(tsv, w.ix, 0, list(reversed(ref.abi_rows(rows))), D, F)   # (the writer sorts)
    want_fa, want_tsv = ref.fasta_text(w.g, stem, edited, rows), ref.tsv_text(w.g, edited, rows, D, F)
    assert open(fa).read() == want_fa
    assert open(tsv).read() == want_tsv
    return want_fa, want_tsv, rows


def test_writers(world, tmp_path):
    w = world
    events = [(55, INS, 10, "ACGTTGCATG", 20, 1),                     # the line's 60 letters end inside S
              (90, DEL, 6, "", 30, 0), (93, DEL, 2, "", 12, 0),       # the second is contested
              (121, INS, 2, "GG", 9, 9), (400, DEL, 1, "", 7, 40),    # the last is rejected
              (w.first_b + 20, INS, 3, "TCA", 15, 2),                 # the second sequence's first applied event is an insertion
              (w.first_b + 50, DEL, 4, "", 15, 2), (w.first_b + 61, INS, 1, "A", 3, 0)]
    fa, tsv, rows = _files(w, tmp_path, events, 3, 0.5)
    lines = fa.split("\n")
    assert lines[0] == ">s1|craftA" and lines[1] == w.g.text[:55] + "ACGTT" and lines[2] == "GCATG" + w.g.text[55:90] + w.g.text[96:116]
    assert all(len(ln) == 60 for ln in lines[1:25])
    body = tsv.split("\n")
    assert body[:3] == ["##consensus_min_depth=3", "##consensus_min_freq=0.5", "chrom\tpos\ttype\tlen\tseq\tsupport\tref_span\taf\tstatus\tcons_pos"]
    assert body[3] == "craftA\t55\tINS\t10\tACGTTGCATG\t20\t1\t0.9523\tapplied\t55"
    assert body[4] == "craftA\t90\tDEL\t6\t.\t30\t0\t1.0000\tapplied\t100"
    assert body[5] == "craftA\t93\tDEL\t2\t.\t12\t0\t1.0000\tcontested\t."
    assert body[6] == "craftA\t121\tINS\t2\tGG\t9\t9\t0.5000\tapplied\t125"
    assert body[7] == "craftB\t20\tINS\t3\tTCA\t15\t2\t0.8823\tapplied\t20"
    assert body[8] == "craftB\t50\tDEL\t4\t.\t15\t2\t0.8823\tapplied\t53"
    assert body[9] == "craftB\t61\tINS\t1\tA\t3\t0\t1.0000\tapplied\t60" and body[10:] == [""]
    # a sample without accepted events: the three header lines alone, and the plain consensus
    fa0, tsv0, _ = _files(w, tmp_path, events, 1000, 0.25)
    assert tsv0 == "##consensus_min_depth=1000\n##consensus_min_freq=0.25\n" + body[2] + "\n"
    plain = str(tmp_path / "plain.fa")
    hostlib.write_consensus_fasta(plain, "s1", w.ix, 0, w.letters)
    assert open(plain).read() == fa0


def test_writers_on_random_sets(world, tmp_path):
    rng = random.Random(21)
    for i in range(12):
        D, F = ref.PAIRS[i % 4]
        _files(world, tmp_path, _random_events(rng, world), D, F, "r%d" % i)


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_call_argument_errors(golden_dir, tmp_path):
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    base = [BRONKO, "call", "-d", os.path.join(golden_dir, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")]
    for extra, word in ((["--consensus-indels", "--consensus"], "--consensus-indels needs --indels"),
                        (["--consensus-indels", "--indels"], "--consensus-indels needs --consensus"),
                        (["--consensus-indels"], "--consensus-indels needs")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout and "no HIP device" not in r.stdout, (extra, r.stdout)
        assert not os.path.exists(str(tmp_path / "o" / "x.consensus.fa"))
