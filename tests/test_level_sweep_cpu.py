"""The count-level sweep (tests/level_sweep.py) as an instrument, on the CPU with the oracle alone: what it sees that the plain
pileup comparison does not, that its reference is right at the threshold edges, and that the read sets of
tests/test_gpu_count_levels.py meet its condition (no count above 32)."""
import os

import numpy as np
import pytest

from bronko_amd import synth
from oracle import cross_oracle
from tests import helpers, level_sweep


def _same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays())) and np.array_equal(a.stats, b.stats)
            and np.array_equal(a.present, b.present))


def _table(oracle, k, reads):
    km, ct, _ = oracle.count_kmers(k, reads, ci=1)
    order = np.argsort(km)
    return km[order], ct[order]


def _level_pile(oracle, ix, km, ct, c):
    """What sample_pileup(ci = cx = c) gives, from the count table: map_kmers of the k-mers counted exactly c times."""
    pile = oracle.Pileup(ix)
    sel = ct == np.uint64(c)
    oracle.map_kmers(ix, km[sel], ct[sel], pile)
    return pile


def _from_levels(oracle, ix, piles, ci):
    """What sample_pileup(ci) gives, from the levels: depths are maxima, #k-mers and the per-genome tallies sums, presence an or."""
    out = oracle.Pileup(ix)
    for c, p in piles.items():
        if c >= ci:
            np.maximum(out.fwd_depth, p.fwd_depth, out=out.fwd_depth)
            np.maximum(out.rev_depth, p.rev_depth, out=out.rev_depth)
            out.fwd_nk += p.fwd_nk
            out.rev_nk += p.rev_nk
            out.stats += p.stats
            out.present |= p.present
    return out


def test_one_lost_occurrence_is_mostly_invisible_to_the_pileup_and_visible_to_the_sweep(oracle, golden_dir):
    """hpv.bkdb, helpers.hpv_reads(1500, 5, err=0.005): the largest count is 27.  60 trials (np.random.default_rng(1)) shorten one
    read by one base at one end, so exactly one k-mer occurrence is lost.  Oracle against oracle, what these seeds give:

      plain comparison (four arrays, stats, present) at ci = 1:   28 of 60 trials invisible
      ... at the default ci = 3:                                  32 of 60 invisible
      sweep over ci = cx = c, c in 1..28:                         56 of 60 caught, 24 of the 28 that ci = 1 does not see
      the 4 trials the sweep does not catch: the lost k-mer, mapped alone, touches no cell -- it votes nowhere, nothing
      downstream of the count depends on it (only the k-mer total of the mate file moves, which the sweep compares too)

    Asserted: some trial is invisible at ci = 1; every trial whose lost k-mer touches a cell is caught by the sweep; every trial
    the sweep does not catch lost a k-mer that touches none.  (The figures are a record, not constants of the test.)

    A level whose k-mers are the unmodified set's is not mapped again (map_kmers is a function of the k-mers it is given), and the
    plain views are put together from the levels; both shortcuts are checked against sample_pileup here."""
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    k = 21
    reads = helpers.hpv_reads(1500, 5, err=0.005)
    km0, ct0 = _table(oracle, k, reads)
    levels = level_sweep.sweep_levels(oracle, [reads], k)
    base = {c: _level_pile(oracle, ix, km0, ct0, c) for c in levels}
    for c in (levels[0], levels[len(levels) // 2], levels[-2], levels[-1]):
        assert _same(base[c], oracle.sample_pileup(ix, [reads], ci=c, cx=c)), c
    plain = {ci: oracle.sample_pileup(ix, [reads], ci=ci) for ci in (1, 3)}
    for ci in plain:
        assert _same(plain[ci], _from_levels(oracle, ix, base, ci))
    rng = np.random.default_rng(1)
    invisible = {1: 0, 3: 0}
    caught = masked_caught = voteless = 0
    for trial in range(60):
        i = int(rng.integers(0, len(reads)))
        left = bool(rng.random() < 0.5)
        mod = list(reads)
        mod[i] = reads[i][1:] if left else reads[i][:-1]
        lost = np.uint64(oracle.kmer_to_u64(reads[i][:k] if left else reads[i][-k:]))
        km, ct = _table(oracle, k, mod)
        at0 = int(np.searchsorted(km0, lost))
        before = int(ct0[at0])
        assert km0[at0] == lost and int(ct0.sum()) - int(ct.sum()) == 1                      # exactly one occurrence is lost ...
        want_km, want_ct = (np.delete(km0, at0), np.delete(ct0, at0)) if before == 1 else (km0, ct0.copy())
        if before > 1:
            want_ct[at0] -= np.uint64(1)
        assert np.array_equal(km, want_km) and np.array_equal(ct, want_ct)                   # ... this one, and nothing else moves
        piles = {c: base[c] if np.array_equal(km[ct == np.uint64(c)], km0[ct0 == np.uint64(c)]) else _level_pile(oracle, ix, km, ct, c)
                 for c in levels}
        assert sum(piles[c] is not base[c] for c in levels) == (1 if before == 1 else 2)     # the levels it leaves and enters
        views = {ci: _from_levels(oracle, ix, piles, ci) for ci in (1, 3)}
        if trial < 3:
            for ci in views:
                assert _same(views[ci], oracle.sample_pileup(ix, [mod], ci=ci))
            for c in (before, before - 1 or levels[-1]):
                assert _same(piles[c], oracle.sample_pileup(ix, [mod], ci=c, cx=c))
        hidden = {ci: _same(plain[ci], views[ci]) for ci in (1, 3)}
        for ci in hidden:
            invisible[ci] += hidden[ci]
        seen = any(not _same(base[c], piles[c]) for c in levels)
        alone = oracle.Pileup(ix)
        oracle.map_kmers(ix, np.array([lost], np.uint64), np.ones(1, np.uint64), alone)
        votes = any(a.any() for a in alone.arrays())
        assert seen == votes, "a lost k-mer that %s was %s by the sweep" % ("votes" if votes else "votes nowhere", "caught" if seen else "missed")
        caught += seen
        masked_caught += seen and hidden[1]
        voteless += not votes
    print("invisible at ci=1: %d, at ci=3: %d, caught by the sweep: %d (%d of those invisible at ci=1), lost k-mer votes nowhere: %d" %
          (invisible[1], invisible[3], caught, masked_caught, voteless))
    assert invisible[1] >= 1 and caught >= 1
    ix.close()


def _cross_levels(files, k, mates, levels):
    """The second restatement (oracle/cross_oracle.py: count_kmers + map_kmers) under ci = cx = c for every level c."""
    index, meta = cross_oracle.build_indexes_files(k, [(fn, [(name.encode(), seq) for name, seq in seqs]) for fn, seqs in files])
    out = {}
    for c in levels:
        maps = cross_oracle.initialize_output_maps(meta)
        stats = np.zeros((len(mates), len(meta), 3), np.uint64)
        present = np.zeros((len(mates), len(meta)), np.uint8)
        total = []
        for m, reads in enumerate(mates):
            kmers, st = cross_oracle.count_kmers(reads, k, c, cx=c)
            total.append(st[1])
            for f, e in cross_oracle.map_kmers(kmers, index, meta, k, 2, False, maps).items():
                stats[m, f] = e
                present[m, f] = 1
        flat = [np.array([row for fid, (_, seqs) in enumerate(meta) for (name, _, _) in seqs for row in mp[fid][name]], np.uint64).reshape(-1)
                for mp in maps]
        out[c] = (flat, stats, present, total)
    return out


@pytest.mark.parametrize("n_files", [1, 3])
def test_both_restatements_agree_at_the_threshold_edges(oracle, golden_dir, n_files):
    """count >= ci and count <= cx at equality: the C oracle and the Python restatement agree on every level ci = cx = c of one
    small crafted set (a 400-base slice of HPV16; reads repeated 1, 2, 3, 5 and 8 times, on both strands, some with a
    substitution, two mate files), on one genome and on three overlapping ones that differ by substitutions."""
    g = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))[3000:3400]
    k = 21
    files = [("f0", [("s0", g)])]
    if n_files == 3:
        files += [("f1", [("s1", level_sweep.substitute(g[60:360], 50, 120, 200))]), ("f2", [("s2", level_sweep.substitute(g[120:400], 30, 31, 170))])]
    mates = [[], []]
    for i, (start, times) in enumerate(zip(range(0, 340, 17), [1, 2, 3, 5, 8] * 4)):
        r = g[start:start + 60]
        if i % 3 == 1:
            r = level_sweep.substitute(r, 20 + i)
        if i % 4 == 2:
            r = level_sweep.revcomp(r)
        mates[i % 2] += [r] * times
    ix = oracle.Index.build_mem(k, files)
    levels = level_sweep.sweep_levels(oracle, mates, k)
    assert len(levels) >= 6
    want = _cross_levels(files, k, mates, levels)
    got = level_sweep.oracle_levels(oracle, ix, mates, k)
    for c in levels:
        flat, stats, present, total = want[c]
        for name, a in zip(level_sweep.ARRAYS, flat):
            assert np.array_equal(getattr(got[c], name), a), (c, name)
        assert np.array_equal(got[c].stats, stats) and np.array_equal(got[c].present, present), c
        assert got[c].kmc_stats[:, 1].tolist() == total, c
    assert sum(int(got[c].fwd_nk.sum() + got[c].rev_nk.sum()) > 0 for c in levels) >= 5      # the levels are not vacuous
    ix.close()


def test_the_gpu_read_sets_meet_the_sweeps_condition(oracle, golden_dir):
    """No read set of tests/test_gpu_count_levels.py holds a k-mer more than 32 times (sweep_levels asserts it), none is a
    two-level sweep where the geometry should give many, and the condition does refuse a set that breaks it."""
    from tests import test_gpu_count_levels as t
    g = t.genome()
    for name, k, mates in t.read_sets(g):
        levels = level_sweep.sweep_levels(oracle, mates, k)
        assert len(levels) <= level_sweep.MAX_COUNT + 1, name
        if name.startswith("G"):
            assert len(levels) >= 6, (name, levels)
    with pytest.raises(AssertionError):
        level_sweep.sweep_levels(oracle, [[g[:100]] * 33], 21)
