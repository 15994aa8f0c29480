"""The regional finalize (finalize_vbin_kernel, bk_finalize_lean.hip) runs two workgroups per CU, and every way of cutting its trips
to memory -- the region's IdRecs [id_lo, min(q0 + 63, n_full - 1)] and the E counters of the ids [q0, q0 + 64) staged once, the
dirty k-mers' answers asked for ahead of the counts (DESIGN section 4, K2 lean: tried, measured) -- has to index that slice right.
Integer work: every case equals the CPU oracle bit for bit -- four pileup arrays, statistics, presence flags, the k-mers scanned --
and runs three ways that must agree: the release library, the testing library, and the testing library with
BK_NO_LEAN_FINALIZE=1 (the general finalize).  The shapes are the smallest at which the region's bookkeeping can go wrong: fewer
ids than one region, an id_lo clamped at either end, ids past n_full, a workgroup that owns rows only, records on both sides of a
region boundary, ids that are not simple, answers that say "none" or "several", the three shapes of the row loop (4, 3 and 2 rows
per wave), and two samples' workgroups sharing CUs."""
import contextlib

import numpy as np
import pytest

from bronko_amd import synth
from tests import helpers

pytestmark = pytest.mark.gpu

WAYS = ("release", "testing", "testing BK_NO_LEAN_FINALIZE=1")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@contextlib.contextmanager
def way(name, monkeypatch):
    """Engines created inside bind the library `name` says; NAME=1 behind it is set in the environment meanwhile."""
    from bronko_amd import _ffi
    _ffi.use_testing_library(name != "release")
    env = [w.split("=")[0] for w in name.split()[1:]]
    for v in env:
        monkeypatch.setenv(v, "1")
    try:
        yield
    finally:
        for v in env:
            monkeypatch.delenv(v, raising=False)
        _ffi.use_testing_library(False)


def same_as_oracle(res, pile):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[:len(pile.kmc_stats), 1].tolist() == pile.kmc_stats[:, 1].tolist()    # k-mer occurrences scanned


def same_results(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.present, b.present) and np.array_equal(a.kmer_stats, b.kmer_stats)


def all_ways(monkeypatch, make_engines, run, ways=WAYS):
    """run(engines) -> list of results, once per way on engines made inside that way; the ways' results must be identical."""
    got = {}
    for name in ways:
        with way(name, monkeypatch):
            engs = make_engines()
            try:
                got[name] = run(engs)
            finally:
                for e in reversed(engs):
                    e.close()
    for name in ways[1:]:
        assert len(got[name]) == len(got[ways[0]])
        for a, b in zip(got[ways[0]], got[name]):
            same_results(a, b)


def regional_finalize_applies(k, n_fixed=2):
    """finalize_runs_by_region's conditions on the index, restated (bk_device.h v_layout_span, bk_index_tables.cpp): one genome file
    of one sequence with dense planes and default parameters is given; what is left is a window of more than one bucket, no pseudo
    k-mers (their ids wrap at k = 31 only) and rows of at most 32 counters.  Returns the rows a wave takes per pass, or 0."""
    wstart, W = n_fixed, k - 2 * n_fixed - 1
    omin = min(wstart, k - wstart - W)
    span = max(wstart + W - 1, k - 1 - wstart) - omin + 1
    return 64 // span if (W > 1 and k < 31 and 0 < span <= 32) else 0


def random_reference(n, seed):
    return synth.codes_to_ascii(np.ascontiguousarray((synth.splitmix64(seed, n) >> np.uint64(33)).astype(np.uint8).reshape(1, n) & 3))[0]


def canonical_kmers(seq, k):
    """[(canonical k-mer, it is the reverse complement of the text)] of every position of seq."""
    out = []
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        rc = w.translate(COMP)[::-1]
        out.append((min(w, rc), rc < w))
    return out


def reads_of(ref, n, read_len, seed, err=0.02):
    return synth.codes_to_ascii(synth.single_end_codes(ref, n, read_len, seed, err=err))


@pytest.fixture(scope="module")
def hpv_ix(oracle, golden_dir):
    import os
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def deep(oracle, hpv_ix):
    """20,000 HPV16 reads at 2 % errors and their oracle pileup, computed once."""
    reads = helpers.hpv_reads(20000, seed=411, err=0.02)
    pile = oracle.sample_pileup(hpv_ix, [reads])
    assert int(pile.fwd_depth.max()) > 50
    return reads, pile


def check_small_reference(oracle, monkeypatch, ref, k, n_reads, read_len, seed):
    assert regional_finalize_applies(k)
    ix = oracle.Index.build_mem(k, [("crafted", [("ref", ref)])])
    reads = reads_of(ref, n_reads, read_len, seed)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_depth.max()) > 0 and int(pile.rev_depth.max()) > 0

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], k), helpers.hip_sample(engs[0], [reads], k, batch=(n_reads + 1) // 2)]   # (items; the plane)
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


def test_reference_shorter_than_one_region(oracle, monkeypatch):
    """70 bp at k = 21: 50 reference k-mers, n_full < 64.  One workgroup owns ids and rows, the second rows only; id_lo is clamped at 0
    and at n_full - 1, the ids it can name are fewer than a region's, the K2e part meets ids past n_full."""
    ref = random_reference(70, 4101)
    assert len({c for c, _ in canonical_kmers(ref, 21)}) == 50
    check_small_reference(oracle, monkeypatch, ref, 21, 600, 50, 4102)


@pytest.mark.parametrize("n_kmers", [131, 128, 126])
def test_last_workgroups_around_the_end_of_the_ids(oracle, monkeypatch, n_kmers):
    """64 m + 3, 64 m and 64 m - 2 reference k-mers: the last workgroup with ids has three, all 64 or 62 of them, and the one behind
    it owns only rows q >= n_full (its own ids are all past the end; the ids its rows name start below its q0 or are the one last record)."""
    ref = random_reference(n_kmers + 20, 4110 + n_kmers)
    assert len({c for c, _ in canonical_kmers(ref, 21)}) == n_kmers
    check_small_reference(oracle, monkeypatch, ref, 21, 1500, 75, 4120 + n_kmers)


def test_repeats_and_near_repeats_across_a_region_boundary(oracle, monkeypatch):
    """A crafted reference of 559 bp: a stretch S of 64 bp three times, the third reverse-complemented (ids that are not simple:
    lean_e_list), its first copy over the ids 40 ... 83 -- on both sides of the boundary between the first two regions --, and a
    stretch T of 50 bp again with one and with two substitutions (reference k-mers one and two bases from each other: dirty ids,
    answers that say "several" or "none": the deferred list)."""
    k = 21
    rnd = random_reference(400, 4130)
    S, T = rnd[0:64], rnd[64:114]
    T1 = bytearray(T); T1[25] = ord("A") if T1[25] != ord("A") else ord("C"); T1 = bytes(T1)
    T2 = bytearray(T1); T2[31] = ord("G") if T2[31] != ord("G") else ord("T"); T2 = bytes(T2)
    ref = rnd[120:160] + S + rnd[160:190] + T + rnd[190:215] + S + rnd[215:245] + T1 + rnd[245:275] + S.translate(COMP)[::-1] + rnd[275:300] + T2 + rnd[300:337]
    assert len(ref) == 559 and ref[40:104] == S
    # the FASTA really has what the case is about: k-mers that occur more than once, in both orientations, and k-mers one base apart
    km = canonical_kmers(ref, k)
    occ = {}
    for i, (c, rc) in enumerate(km):
        occ.setdefault(c, []).append((i, rc))
    in_s = [km[i][0] for i in range(40, 40 + 64 - k + 1)]                       # S's own k-mers, at their first copy
    assert all(len(occ[c]) == 3 and len({rc for _, rc in occ[c]}) == 2 for c in in_s)
    assert len({km[i][0] for i in range(84)}) == 84                            # (no repeat before or among them: ids are positions up to 83)
    t0, t1 = ref.index(T), ref.index(T1)
    assert sum(a != b for a, b in zip(ref[t0 + 10:t0 + 10 + k], ref[t1 + 10:t1 + 10 + k])) == 1
    assert regional_finalize_applies(k) == 3
    ix = oracle.Index.build_mem(k, [("crafted", [("ref", ref)])])
    reads = reads_of(ref, 6000, 100, 4131)
    pile = oracle.sample_pileup(ix, [reads])
    cells = [(40 + 30) * 4, (ref.index(T1) + 25) * 4]                           # inside S's first copy, at T1's substitution
    assert all(int(pile.fwd_depth[c:c + 4].max()) > 20 for c in cells)

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], k), helpers.hip_sample(engs[0], [reads], k, batch=2500)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


def test_smallest_launches(oracle, hpv_ix, monkeypatch):
    """1, 64 and 65 reads of HPV16: nearly every region without an item, every record and E counter read all the same."""
    reads = helpers.hpv_reads(65, seed=401, err=0.02)
    sets = [reads[:1], reads[:64], reads]
    piles = [oracle.sample_pileup(hpv_ix, [r]) for r in sets]
    assert piles[0].kmc_stats[0, 1] == 130

    def run(engs):
        out = [helpers.hip_sample(engs[0], [r], 21) for r in sets]
        for res, pile in zip(out, piles):
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_items_and_planes(oracle, hpv_ix, deep, monkeypatch):
    """20,000 reads at 2 % errors as one launch (the items' instantiation, rows touched by Level 2), as two and as four launches
    (the plane's instantiation), two mate files; and the testing library with BK_NO_FUSE=1 (every launch through the plane)."""
    a, pa = deep
    gm, isnv = synth.sample_genome(synth.read_fasta_bytes(helpers.GOLDEN + "/HPV16.fa"), 9)
    c1, c2 = synth.paired_codes(gm, 7000, 150, 413, isnv=isnv)
    mates = [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]
    pm = oracle.sample_pileup(hpv_ix, mates)

    def run(engs):
        e = engs[0]
        out = [helpers.hip_sample(e, [a], 21), helpers.hip_sample(e, [a], 21, batch=10000), helpers.hip_sample(e, [a], 21, batch=5000),
               helpers.hip_sample(e, mates, 21)]
        for res, pile in zip(out, (pa, pa, pa, pm)):
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run, WAYS + ("testing BK_NO_FUSE=1",))


@pytest.mark.parametrize("k", [19, 29])
def test_other_row_shapes(oracle, golden_dir, monkeypatch, k):
    """k = 19: rows of 15 counters, four per wave and six passes; k = 29: rows of 25, two per wave and twelve passes, the most there are (k = 21, everywhere else in this file: rows of 17, three per wave, eight passes)."""
    import os
    assert regional_finalize_applies(k) == {19: 4, 29: 2}[k] and regional_finalize_applies(21) == 3
    ix = oracle.Index.build(k, [os.path.join(golden_dir, "HPV16.fa")])
    reads = helpers.hpv_reads(6000, seed=430 + k, err=0.02)
    pile = oracle.sample_pileup(ix, [reads])

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], k), helpers.hip_sample(engs[0], [reads], k, batch=2500)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


def test_count_thresholds_that_bite(oracle, hpv_ix, deep, monkeypatch):
    """ci = 2 and cs = 40, below the deepest count of the sample: the E counters and the rows' sums under -ci / -cs that bite."""
    from bronko_amd import Params
    a, pa = deep
    assert int(max(pa.fwd_depth.max(), pa.rev_depth.max())) > 40
    pile = oracle.sample_pileup(hpv_ix, [a], ci=2, cs=40)
    assert int(max(pile.fwd_depth.max(), pile.rev_depth.max())) == 40
    assert int(pile.fwd_nk.sum()) > int(pa.fwd_nk.sum())                       # (k-mers seen twice count now)

    def run(engs):
        out = [helpers.hip_sample(engs[0], [a], 21), helpers.hip_sample(engs[0], [a], 21, batch=10000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix, Params(ci=2, cs=40))], run)


def test_four_engines_in_turn(oracle, hpv_ix, deep, monkeypatch):
    """An engine and three forks run the 20,000-read sample on their own streams, all begun before any is finished: two samples'
    finalize workgroups share CUs.  Every engine's result is the oracle's."""
    from bronko_amd import pack_reads
    a, pa = deep
    words, lens = pack_reads(a, 21)

    def make():
        eng = helpers.engine_from_oracle_index(hpv_ix)
        return [eng, eng.fork(), eng.fork(), eng.fork()]

    def run(engs):
        out = []
        for _ in range(2):
            for e in engs:
                e.sample_begin()
                e.push_reads(0, words, lens)
            for e in engs:
                e.sample_finalize(1)
            out += [e.sample_download(1) for e in engs]
        for res in out:
            same_as_oracle(res, pa)
        return out

    all_ways(monkeypatch, make, run)
