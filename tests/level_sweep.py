"""Count-level sweeps (tests/ only): the scan's per-k-mer counts observed through the public C ABI.

A pileup depth is the MAXIMUM of the counts of the k-mers that vote at a cell and the #k-mers arrays only say that a k-mer passed
-ci, so a k-mer counted c - 1 instead of c mostly changes nothing.  Under ci = cx = c only the k-mers whose count is exactly c vote:
the #k-mers arrays then list them cell by cell, and a miscounted k-mer shows up at the wrong level.  level_sweep runs one read set
once per count value that occurs in it (forks of one parent engine carry the thresholds) and compares every level with the oracle.

Also here: the crafted read sets of tests/test_gpu_count_levels.py (set G: chunk and read geometry, set T: tiles and the deal), so
that tests/test_level_sweep_cpu.py can check them against the sweep's own condition without a GPU.
"""
import numpy as np

from tests import helpers

MAX_COUNT = 32          # no read set of a sweep holds a k-mer more often: at most MAX_COUNT + 1 levels
COMP = bytes.maketrans(b"ACGT", b"TGCA")
ARRAYS = ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk")


def revcomp(r):
    return bytes(r).translate(COMP)[::-1]


# ---- the instrument --------------------------------------------------------------------------------------------------------------
def sweep_levels(oracle, mates, k):
    """The levels of a read set: every count value of the oracle's count table of each mate file, and the largest + 1 (at which
    nothing may vote).  A set that holds no k-mer, or one more than MAX_COUNT times, is not a sweep's."""
    counts = set()
    for reads in mates:
        counts.update(int(c) for c in np.unique(oracle.count_kmers(k, reads, ci=1)[1]))
    assert counts, "the read set holds no k-mer: nothing to sweep"
    assert max(counts) <= MAX_COUNT, "a k-mer occurs %d times: spread the reads or split the set (at most %d)" % (max(counts), MAX_COUNT)
    return sorted(counts) + [max(counts) + 1]


def oracle_levels(oracle, ix, mates, k, **window_params):
    """{level: the oracle's Pileup under ci = cx = level}: computed once per read set, shared by every engine path that runs it."""
    assert ix.k == k
    levels = sweep_levels(oracle, mates, k)
    exp = {c: oracle.sample_pileup(ix, mates, ci=c, cx=c, **window_params) for c in levels}
    top = exp[levels[-1]]
    assert not any(a.any() for a in top.arrays()) and not top.stats.any() and not top.present.any(), "the oracle votes above the largest count"
    assert any(exp[c].fwd_nk.any() or exp[c].rev_nk.any() for c in levels[:-1]), "no level votes anywhere: the sweep would be vacuous"
    return exp


def assert_same_level(oracle, ix, res, pile, selected_only=False):
    """helpers.assert_same_pileup plus the k-mer occurrences scanned; under pileup_selected_only the statistics of every genome
    and the rows of the selected genome only, every other row zero."""
    if selected_only:
        assert np.array_equal(res.stats, pile.stats), (res.stats.tolist(), pile.stats.tolist())
        assert np.array_equal(res.present, pile.present)
        best = oracle.pick_best_genome(ix, pile.stats.sum(axis=0), pile.present.max(axis=0))
        lo, n = ix.genome_cells(best) if best >= 0 else (0, 0)
        for name in ARRAYS:
            got, ref = getattr(res, name), getattr(pile, name)
            sel = slice(lo * 4, (lo + n) * 4)
            if not np.array_equal(got[sel], ref[sel]):
                bad = np.nonzero(got[sel] != ref[sel])[0]
                raise AssertionError("%s of the selected genome %d differs in %d cells; first at %d: hip=%d oracle=%d" %
                                     (name, best, len(bad), lo * 4 + bad[0], got[sel][bad[0]], ref[sel][bad[0]]))
            assert not got[:lo * 4].any() and not got[(lo + n) * 4:].any(), "%s: rows of a genome that was not selected" % name
    else:
        helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[:, 1].tolist() == pile.kmc_stats[:, 1].tolist(), ("k-mer occurrences", res.kmer_stats[:, 1], pile.kmc_stats[:, 1])


def level_sweep(oracle, ix, parent_engine, mates, k, expected=None, run=None, pileup_selected_only=False, **window_params):
    """One fork of parent_engine per level c with Params(ci=c, cx=c, ...), the sample through helpers.hip_sample, against
    oracle.sample_pileup(ix, mates, ci=c, cx=c, ...) -- all four arrays, stats, present and the k-mer total of every mate file.
    expected: oracle_levels(...) of this read set, when several engine paths share it.  run(engine) -> [results]: how the sample
    is pushed (default: one push per mate file, once); every result it returns is compared.  window_params: n_fixed /
    use_full_kmer, the parent's.  Returns the levels."""
    from bronko_amd import Params
    if expected is None:
        expected = oracle_levels(oracle, ix, mates, k, **window_params)
    levels = sorted(expected)
    assert 2 <= len(levels) <= MAX_COUNT + 1 and levels[-1] <= MAX_COUNT + 1
    if run is None:
        run = lambda e: [helpers.hip_sample(e, mates, k)]
    for c in levels:
        fork = parent_engine.fork(Params(ci=c, cx=c, pileup_selected_only=pileup_selected_only, **window_params))
        try:
            for i, res in enumerate(run(fork)):
                try:
                    assert_same_level(oracle, ix, res, expected[c], pileup_selected_only)
                    if c == levels[-1]:
                        assert not any(a.any() for a in res.arrays()) and not res.stats.any(), "votes above the largest count"
                except AssertionError as e:
                    raise AssertionError("level ci = cx = %d of %s, sample %d of the fork: %s" % (c, levels, i, e)) from None
        finally:
            fork.close()
    return levels


# ---- set G: chunk and read geometry ----------------------------------------------------------------------------------------------
G_LENGTHS = (21, 22, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 159, 160, 161, 181, 255, 256, 257, 287, 288, 289, 300)
G_BOUNDARIES = (128, 160, 256, 288)    # read offsets at which the scan's chunks, carries and flag words change over
G_PAIR_LENGTH = 300


def substitute(read, *positions):
    r = bytearray(read)
    for p in positions:
        r[p] = b"ACGT"[(b"ACGT".index(r[p]) + 1 + p % 3) & 3]
    return bytes(r)


def g_positions(L, k):
    """Read offsets of set G's single substitutions in a read of L bases."""
    if L <= 65:
        return list(range(L))
    ps = set(range(0, k + 1)) | set(range(L - (k + 1), L))
    for b in G_BOUNDARIES:
        ps |= set(range(b - (k + 1), b + (k + 1) + 1))
    return sorted(p for p in ps if 0 <= p < L)


class _Strider:
    """Read starts striding through the genome: every read at another reference offset, so that counts stay small (the geometry
    that matters is relative to the read)."""

    def __init__(self, genome, stride):
        self.g, self.stride, self.at = genome, stride, 0

    def take(self, L):
        s = self.at % (len(self.g) - L + 1)
        self.at += self.stride
        return self.g[s:s + L]


def _both_ends(genome):
    """Reads that contain the reference's first and last k-mer, in both orientations."""
    return [genome[:150], revcomp(genome[:150]), genome[-150:], revcomp(genome[-150:])]


def set_g(genome, k, lengths=G_LENGTHS):
    """For each length the exact read and one read per single substitution (g_positions), each in both orientations and each at
    a reference offset of its own."""
    st = _Strider(genome, 61)
    reads = _both_ends(genome)
    for L in lengths:
        for p in [None] + g_positions(L, k):
            for rc in (False, True):
                r = st.take(L)
                if p is not None:
                    r = substitute(r, p)
                reads.append(revcomp(r) if rc else r)
    return reads


def set_g_pairs(genome, k, every=1):
    """Two substitutions at distances 1, 2, 3, k - 1, k, k + 1, every placement that straddles one of the boundaries (the first
    below it, the second at or above it): Level 2's two-difference path.  Both orientations.  every = n: every n-th placement."""
    st = _Strider(genome, 97)
    reads = _both_ends(genome)
    i = 0
    for b in G_BOUNDARIES:
        for d in (1, 2, 3, k - 1, k, k + 1):
            for p in range(b - d, b):
                if p < 0 or p + d >= G_PAIR_LENGTH:
                    continue
                i += 1
                if i % every:
                    continue
                for rc in (False, True):
                    r = substitute(st.take(G_PAIR_LENGTH), p, p + d)
                    reads.append(revcomp(r) if rc else r)
    return reads


def set_g_parts(genome, k):
    """Set G, whole, as the read sets that meet the MAX_COUNT condition: three by every third length, and the pairs."""
    return [set_g(genome, k, G_LENGTHS[j::3]) for j in range(3)] + [set_g_pairs(genome, k)]


# ---- set T: tiles and the deal ---------------------------------------------------------------------------------------------------
def set_t(genome, n, read_len=32, stride=5):
    """n reads of 32 bases cycling over the genome, every seventh against it."""
    span = len(genome) - read_len + 1
    out = []
    for i in range(n):
        s = (i * stride) % span
        r = genome[s:s + read_len]
        out.append(revcomp(r) if i % 7 == 3 else r)
    return out
