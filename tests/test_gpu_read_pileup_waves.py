"""merged_add of read_pileup_count_kernel (bk_read_pileup.hip) on waves of a fixed composition.  A store of at most 64 rows is one wave
whatever order the rows land in, so a case is a multiset of rows: groups of equal (strand, first cell, end) of chosen sizes, more
groups than the wave has merge rounds, pairs, one row apart from 63, partial waves whose live rows sit at cell 0 (a dead lane carries
index 0), rows that share their end and differ in length, one substitution shared by rows of both strands at several distances from
their ends and in several mismatch slots.  Twice the multiset is two waves of one workgroup that add to the same words.  The reads are
exact stretches of the crafted genome with planted substitutions; tests/linkage_ref.py places them (the row count and the groups are
asserted on the restatement, so no case goes vacuous) and every counter of every cell must equal tests/read_pileup_ref.py, at an end
distance with 2E < n and at one with 2E >= n."""
from collections import Counter

import pytest

from tests import indels_ref, linkage_ref
from tests.test_gpu_read_pileup import Crafted, _check, _sample

pytestmark = pytest.mark.gpu
K = 21
N = 100                                                            # the usual row: E = 10 leaves two stretches, E = 50 and 60 none


@pytest.fixture(scope="module")
def crafted():
    c = Crafted(K)
    yield c
    c.eng.close()
    c.ix.close()


def _read(a, c0, n, rev=False, subs=()):
    """n letters of `a` from cell c0 on; subs: offsets (the next letter is put there) or (offset, letter); then against the reference"""
    s = list(a[c0:c0 + n])
    for sub in subs:
        off, to = sub if isinstance(sub, tuple) else (sub, "ACGT"[("ACGT".index(s[sub]) + 1) % 4])
        assert s[off] != to and s[off] in "ACGT"
        s[off] = to
    s = "".join(s)
    return indels_ref.revcomp(s) if rev else s


def _groups(rows):
    """sizes of the groups of equal (strand, first cell, end), largest first"""
    return sorted(Counter((r[2], r[0], r[0] + r[1]) for r in rows).values(), reverse=True)


def _run(c, reads, ends, times, groups, what):
    reads = list(reads) * times
    assert len(reads) <= 64 * times and (times == 1 or 65 <= len(reads) <= 128)
    rows, _ = linkage_ref.link_rows(c.g, reads, 8)
    assert len(rows) == len(reads) and _groups(rows) == [times * x for x in groups], (what, len(rows), _groups(rows))
    _sample(c.eng, reads, c.k)
    assert len(c.eng.download_link_rows()) == len(rows)
    assert any(2 * E < min(r[1] for r in rows) for E in ends) and any(2 * E >= max(r[1] for r in rows) for E in ends)
    return rows, [_check(c.eng, c.ix, c.g, rows, E, what) for E in ends]


def _grouped(a, sizes, step=7):
    """len(sizes) groups of equal rows: group g of sizes[g] copies at cell 700 + step * g, the strands alternating"""
    return [_read(a, 700 + step * g, N, rev=bool(g & 1)) for g, size in enumerate(sizes) for _ in range(size)]


COMPOSITIONS = {"eight groups of eight": [8] * 8,                  # more groups than rounds: the rounds run out, the rest take single adds
                "thirty-two pairs": [2] * 32,
                "sixty-three and one": [63, 1],
                "sixty-four distinct": [1] * 64,                   # the first leader stands alone: no second round
                "three large groups and two pairs": [20, 20, 20, 2, 2]}


@pytest.mark.parametrize("times", [1, 2], ids=["one wave", "two waves"])
@pytest.mark.parametrize("name", list(COMPOSITIONS))
def test_groups_of_equal_rows(crafted, name, times):
    c, sizes = crafted, COMPOSITIONS[name]
    a = c.seqs[0][1]
    rows, (at10, _, _) = _run(c, _grouped(a, sizes, 3 if len(sizes) > 40 else 7), (10, 50, 60), times, sorted(sizes, reverse=True), name)
    first = Counter((r[0], r[2]) for r in rows)
    for (c0, strand), count in first.items():                      # a first cell is no other row's: its counter is the group's size
        ref = "ACGT".index(a[c0])
        assert at10[c0, 4 * strand + ref] == sum(v for (x, s), v in first.items() if s == strand and x <= c0 < x + N)
        assert at10[c0, 8 + ref] >= count


@pytest.mark.parametrize("n_rows,times", [(2, 1), (33, 1), (63, 1), (33, 2), (63, 2)])
def test_a_partial_wave_whose_rows_begin_at_cell_zero(crafted, n_rows, times):
    """The dead lanes of the wave hold index 0 in every add, and so do the live ones here: the forward strand's cover at cell 0, the
    near-end cover at cell 0, and word 0 of mm and of mm_near, which is a forward row's substitution to A at cell 0."""
    c = crafted
    a = c.seqs[0][1]
    assert a[0] != "A"
    other = next(x for x in "CGT" if x != a[0])
    kinds = [dict(n=N, subs=((0, "A"),)), dict(n=N, rev=True), dict(n=N), dict(n=N + 20, subs=((0, "A"), 40)), dict(n=N + 20, rev=True, subs=((0, other),))]
    reads = [_read(a, 0, **kinds[i % 5]) for i in range(n_rows)]
    rows, (at10, at50, _) = _run(c, reads, (10, 50, 60), times, _groups(linkage_ref.link_rows(c.g, reads, 8)[0]), n_rows)
    assert all(r[0] == 0 for r in rows) and {r[2] for r in rows} == {0, 1}
    fwd, to_a = sum(1 for r in rows if r[2] == 0), sum(1 for r in rows if r[2] == 0 and (0, 0) in r[3])
    assert to_a >= 1 and len(rows) == n_rows * times
    ref = "ACGT".index(a[0])
    for got in (at10, at50):
        assert got[0, 0] == to_a and got[0, ref] == fwd - to_a and got[0, :8].sum() == len(rows) and got[0, 8:].sum() == len(rows) and got[0, 8] == to_a


def test_a_partial_wave_of_two_rows_at_cell_zero_twice_is_still_one_wave(crafted):
    c = crafted
    a = c.seqs[0][1]
    reads = [_read(a, 0, N, subs=((0, "A"),)), _read(a, 0, N, rev=True)] * 2
    rows, (at10, _) = _run(c, reads, (10, 50), 1, [2, 2], "four rows")
    assert at10[0, 0] == 2 and at10[0, :8].sum() == 4


@pytest.mark.parametrize("times", [1, 2], ids=["one wave", "two waves"])
def test_rows_that_share_their_end_and_differ_in_length(crafted, times):
    """At E = 50 the row of 80 cells is near an end everywhere -- the -1 of its near-end stretch goes to its end -- and the row of 140
    is not: its -1 goes to first cell + E, then +1 to end - E and -1 to the end.  The row of 100 is the border, n = 2E."""
    c = crafted
    a = c.seqs[0][1]
    end = 840
    reads = [_read(a, end - n, n, rev=bool(i & 1)) for i, n in enumerate([140] * 20 + [80] * 20 + [100] * 12 + [101] * 6 + [99] * 6)]
    rows, (at10, at50, at70) = _run(c, reads, (10, 50, 70), times, [10] * 4 + [6] * 2 + [3] * 4, "a shared end")
    assert {r[0] + r[1] for r in rows} == {end}
    near = lambda got, cell: int(got[cell, 8:].sum())
    assert near(at50, end - 1) == 64 * times and near(at50, end - 70) == 44 * times      # (70 from the end: every row but those of 140 cells)
    assert near(at10, end - 70) == 0 and near(at70, end - 70) == 64 * times and near(at50, end - 140) == 20 * times


@pytest.mark.parametrize("times", [1, 2], ids=["one wave", "two waves"])
def test_one_substitution_near_an_end_of_some_rows_and_not_of_others(crafted, times):
    """64 rows over cell 800 that all carry the same letter there, 40 along and 24 against the reference, at 5, 20 and 60 cells from
    their first cell: the mm words of the cell are merged over the whole wave, the mm_near word over those lanes whose row is near."""
    c = crafted
    a = c.seqs[0][1]
    cell = 800
    starts = [cell - 5] * 22 + [cell - 20] * 22 + [cell - 60] * 20
    reads = [_read(a, c0, N, rev=i % 8 >= 5, subs=(cell - c0,)) for i, c0 in enumerate(starts)]
    ends = (10, 20, 30, 50)                                        # (E = 20: the rows that carry it 20 cells from their first are not near)
    rows, got = _run(c, reads, ends, times, _groups(linkage_ref.link_rows(c.g, reads, 8)[0]), "one substitution")
    assert sum(1 for r in rows if r[2] == 0) == 40 * times and all(len(r[3]) == 1 for r in rows)
    b = ("ACGT".index(a[cell]) + 1) % 4
    for E, cells in zip(ends, got):
        assert cells[cell, b] == 40 * times and cells[cell, 4 + b] == 24 * times and cells[cell, :8].sum() == 64 * times
        assert cells[cell, 8 + b] == {10: 22, 20: 22, 30: 44, 50: 64}[E] * times == cells[cell, 8:].sum()


@pytest.mark.parametrize("times", [1, 2], ids=["one wave", "two waves"])
def test_one_substitution_in_the_first_mismatch_slot_of_some_rows_and_the_fourth_of_others(crafted, times):
    """The adds to one mm word fall in different turns of the slot loop: they are not merged, and they add up all the same."""
    c = crafted
    a = c.seqs[0][1]
    c0, off = 790, 60
    kinds = [(off,), (30, 40, 50, off), (30, off), (off, 70), (30, 40, 50, off, 70)]
    reads = [_read(a, c0, N, rev=i % 3 == 2, subs=kinds[i % 5]) for i in range(60)]
    rows, got = _run(c, reads, (10, 45, 50), times, _groups(linkage_ref.link_rows(c.g, reads, 8)[0]), "slots")
    assert {[o for o, _ in r[3]].index(off) for r in rows} == {0, 1, 3}
    nxt = lambda cell: ("ACGT".index(a[cell]) + 1) % 4
    for E, cells in zip((10, 45, 50), got):                        # (39 cells from the end: near from E = 40 on)
        assert cells[c0 + off, nxt(c0 + off)] + cells[c0 + off, 4 + nxt(c0 + off)] == 60 * times
        assert cells[c0 + off, 8 + nxt(c0 + off)] == (0 if E == 10 else 60 * times)
        assert cells[c0 + 30, :8].sum() == 60 * times and cells[c0 + 30, nxt(c0 + 30)] + cells[c0 + 30, 4 + nxt(c0 + 30)] == 36 * times
