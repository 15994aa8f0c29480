"""The E bins of a binned-scan launch are counted inside the Level 2 launch that follows it (launch_level2's ride) instead of in
a bin_count_kernel launch of their own.  Integer work: every case equals the CPU oracle bit for bit -- four pileup arrays,
statistics, presence flags, the k-mers scanned -- and runs three ways that must agree: the release library, the testing library,
and the testing library with BK_NO_E_RIDE=1 (the launches as they were before the ride)."""
import contextlib
import os

import numpy as np
import pytest

from bronko_amd import synth
from tests import helpers

pytestmark = pytest.mark.gpu

WAYS = ("release", "testing", "testing BK_NO_E_RIDE=1")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@contextlib.contextmanager
def way(name, monkeypatch):
    """Engines created inside bind the library `name` says, with or without the ride."""
    from bronko_amd import _ffi
    _ffi.use_testing_library(name != "release")
    if name.endswith("BK_NO_E_RIDE=1"):
        monkeypatch.setenv("BK_NO_E_RIDE", "1")
    try:
        yield
    finally:
        monkeypatch.delenv("BK_NO_E_RIDE", raising=False)
        _ffi.use_testing_library(False)


def same_as_oracle(res, pile):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[:len(pile.kmc_stats), 1].tolist() == pile.kmc_stats[:, 1].tolist()    # k-mer occurrences scanned


def same_results(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.present, b.present) and np.array_equal(a.kmer_stats, b.kmer_stats)


def three_ways(monkeypatch, make_engines, run):
    """run(engines) -> list of results, once per way on engines made inside that way; the ways' results must be identical."""
    got = {}
    for name in WAYS:
        with way(name, monkeypatch):
            engs = make_engines()
            try:
                got[name] = run(engs)
            finally:
                for e in reversed(engs):
                    e.close()
    for name in WAYS[1:]:
        assert len(got[name]) == len(got[WAYS[0]])
        for a, b in zip(got[WAYS[0]], got[name]):
            same_results(a, b)


@pytest.fixture(scope="module")
def hpv_ix(oracle, golden_dir):
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def hpv_genome():
    return synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))


def test_smallest_launches(oracle, hpv_ix, monkeypatch):
    """1, 64 and 65 reads -- one scan workgroup, a partial second tile, nearly every E bin empty: the ride's workgroups outnumber
    Level 2's own -- and a sample whose only reads are shorter than k: nothing is launched, nothing waits on an empty grid."""
    reads = helpers.hpv_reads(65, seed=301, err=0.02)
    sets = [reads[:1], reads[:64], reads, [b"ACGT" * 5, b"A" * 20, b"", b"ACGTN" * 4]]
    piles = [oracle.sample_pileup(hpv_ix, [r]) for r in sets]
    assert piles[3].kmc_stats[0, 1] == 0 and piles[0].kmc_stats[0, 1] == 130 and int(piles[2].fwd_depth.max() + piles[2].rev_depth.max()) > 0

    def run(engs):
        out = [helpers.hip_sample(engs[0], [r], 21) for r in sets]
        for res, pile in zip(out, piles):
            same_as_oracle(res, pile)
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_level2_busy_while_the_e_bins_count(oracle, hpv_ix, hpv_genome, monkeypatch):
    """20,000 reads with 2 % errors (plenty of close pairs: Level 2 has work while the E bins count): as one launch (the ride with
    V items waiting: no bin_count_kernel at all), as two and as four launches of one mate file (the later ones: bin_count_kernel
    over the V bins, then the ride), two mate files, and a sample begun, pushed and abandoned followed by two more on the same
    engine (the overflow count's parity and the waiting items across samples)."""
    from bronko_amd import pack_reads
    a = helpers.hpv_reads(20000, seed=311, err=0.02)
    b = helpers.hpv_reads(6000, seed=312, with_n=True, ragged=True)
    gm, isnv = synth.sample_genome(hpv_genome, 9)
    c1, c2 = synth.paired_codes(gm, 7000, 150, 313, isnv=isnv)
    mates = [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]
    pa, pb, pm = oracle.sample_pileup(hpv_ix, [a]), oracle.sample_pileup(hpv_ix, [b]), oracle.sample_pileup(hpv_ix, mates)
    assert int(pa.fwd_depth.max()) > 50

    def run(engs):
        e = engs[0]
        out = [helpers.hip_sample(e, [a], 21), helpers.hip_sample(e, [a], 21, batch=10000), helpers.hip_sample(e, [a], 21, batch=5000),
               helpers.hip_sample(e, mates, 21)]
        e.sample_begin()                       # abandoned with E bins counted, V items waiting and rows noted
        e.push_reads(0, *pack_reads(a, 21))
        out += [helpers.hip_sample(e, [b], 21), helpers.hip_sample(e, [a], 21)]
        for res, pile in zip(out, (pa, pa, pa, pm, pb, pa)):
            same_as_oracle(res, pile)
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_a_hot_bin_through_bucket_extension_and_overflow_list(oracle, hpv_ix, hpv_genome, monkeypatch):
    """30,000 copies of one read that carries one substitution, on both strands: thirty scan workgroups with about a thousand
    items per bin each -- beyond the 48-slot bucket and the 256-slot extension, well inside the overflow list, which every
    riding E bin reads through.  Depths of 20,000 and 10,000 at the substitution."""
    w = bytearray(hpv_genome[2000:2150].upper())
    w[75] = ord("A") if w[75] != ord("A") else ord("C")
    w = bytes(w)
    reads = [w] * 20000 + [w.translate(COMP)[::-1]] * 10000
    pile = oracle.sample_pileup(hpv_ix, [reads])
    sub = (2000 + 75) * 4 + b"ACGT".index(bytes([w[75]]))                        # the substituted base's cell of the pileup
    assert int(pile.fwd_depth[sub]) == 20000 and int(pile.rev_depth[sub]) == 10000

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], 21), helpers.hip_sample(engs[0], [reads], 21, batch=17000)]
        for res in out:
            same_as_oracle(res, pile)
            assert int(res.fwd_depth[sub]) == 20000 and int(res.rev_depth[sub]) == 10000
            assert int(res.fwd_depth.max()) == 20000 and int(res.rev_depth.max()) == 10000
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_the_planned_grid_together_with_the_ride(oracle, hpv_ix, hpv_genome, monkeypatch):
    """A family of four (an engine and three forks: l2_plan_kernel is on).  On-target reads leave the plan at its floor -- most of
    Level 2's workgroups leave at once, by the planned share of Level 2's OWN block count --; 40,000 reads at 5 % errors mark
    more than 32,768 records and raise it above the floor.  Every engine of the family runs both samples."""
    gm, isnv = synth.sample_genome(hpv_genome, 5)
    on_target = synth.codes_to_ascii(synth.single_end_codes(gm, 12000, 150, 321, err=0.005, isnv=isnv))
    noisy = synth.codes_to_ascii(synth.single_end_codes(gm, 40000, 150, 322, err=0.05, isnv=isnv))
    p_on, p_noisy = oracle.sample_pileup(hpv_ix, [on_target]), oracle.sample_pileup(hpv_ix, [noisy])

    def make():
        eng = helpers.engine_from_oracle_index(hpv_ix)
        return [eng, eng.fork(), eng.fork(), eng.fork()]

    def run(engs):
        out = []
        for e in engs:
            out += [helpers.hip_sample(e, [on_target], 21), helpers.hip_sample(e, [noisy], 21)]
        for i, res in enumerate(out):
            same_as_oracle(res, p_noisy if i & 1 else p_on)
        return out

    three_ways(monkeypatch, make, run)


@pytest.mark.parametrize("k", [31, 19])
def test_other_k(oracle, golden_dir, monkeypatch, k):
    """level2_kernel<., 31, .> and the k-at-run-time instantiation carry the ride too."""
    ix = oracle.Index.build(k, [os.path.join(golden_dir, "HPV16.fa")])
    reads = helpers.hpv_reads(6000, seed=330 + k, err=0.02)
    pile = oracle.sample_pileup(ix, [reads])

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], k), helpers.hip_sample(engs[0], [reads], k, batch=2500)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


def test_full_kmer_stats(oracle, hpv_ix, hpv_genome, monkeypatch):
    """The statistics instantiations (level2_kernel<true, ., .>): the ride next to a Level 2 that fills the k-mer table."""
    from bronko_amd import Params
    gm, isnv = synth.sample_genome(hpv_genome, 6)
    c1, c2 = synth.paired_codes(gm, 5000, 150, 341, err=0.01, isnv=isnv)
    junk = synth.codes_to_ascii(np.ascontiguousarray(synth.splitmix64(77, 300 * 150).astype(np.uint8).reshape(300, 150) & 3))
    mates = [synth.codes_to_ascii(c1) + junk, synth.codes_to_ascii(c2)]
    pile = oracle.sample_pileup(hpv_ix, mates)

    def run(engs):
        out = [helpers.hip_sample(engs[0], mates, 21), helpers.hip_sample(engs[0], mates, 21, batch=2000)]
        for res in out:
            same_as_oracle(res, pile)
            for col in (2, 3):                                                   # unique / unique counted k-mers
                assert res.kmer_stats[:, col].tolist() == pile.kmc_stats[:, col].tolist()
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix, Params(full_kmer_stats=True, kmer_table_log2=20))], run)


def test_four_genomes_have_no_waiting_v_items(oracle, sars_paths, monkeypatch):
    """A multi-file index (four SARS-CoV-2 genomes, 15,000 pairs): no V items wait, nbatch_kernel keeps its own launch in front --
    bin_count_kernel over the V bins, then Level 2 with the ride, for every launch."""
    ix = oracle.Index.build(21, sars_paths)
    gm, isnv = synth.sample_genome(synth.read_fasta_bytes(sars_paths[2]), 3)
    c1, c2 = synth.paired_codes(gm, 15000, 150, 3, isnv=isnv)
    mates = [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]
    pile = oracle.sample_pileup(ix, mates)

    def run(engs):
        out = [helpers.hip_sample(engs[0], mates, 21), helpers.hip_sample(engs[0], mates, 21, batch=6000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()
