"""A sample's outputs -- the pileup arrays, statistics, presence flags, the deferred counts -- are zeroed by workgroups of the sample's
first Level 2 launch (launch_level2's zero ride) and the k-mer tallies of the next sample with them, instead of by a zero_small_kernel
launch in bk_sample_begin; a sample without a Level 2 launch pays at its finalize.  Integer work: every sample of every case equals the
CPU oracle bit for bit -- four pileup arrays, statistics, presence flags, the k-mers scanned, the records counted -- and every case runs
three ways that must agree in every output of sample_download: the release library, the testing library, and the testing library with
BK_NO_ZERO_RIDE=1 (the launch as it was).  Every case runs at least three samples in a row on one engine, with different reads: a stale
pileup cell, statistics word or k-mer tally of either parity shows in the sample behind it."""
import contextlib
import os

import numpy as np
import pytest

from bronko_amd import pack_reads, synth
from tests import adapter_ref, helpers, primer_ref

pytestmark = pytest.mark.gpu

WAYS = ("release", "testing", "testing BK_NO_ZERO_RIDE=1")
K = 21


@contextlib.contextmanager
def way(name, monkeypatch, env):
    """Engines created inside bind the library `name` says, with or without the ride; env: further testing aids (the release library
    reads none)."""
    from bronko_amd import _ffi
    _ffi.use_testing_library(name != "release")
    if name.endswith("BK_NO_ZERO_RIDE=1"):
        monkeypatch.setenv("BK_NO_ZERO_RIDE", "1")
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    try:
        yield
    finally:
        monkeypatch.delenv("BK_NO_ZERO_RIDE", raising=False)
        for key in env:
            monkeypatch.delenv(key, raising=False)
        _ffi.use_testing_library(False)


def n_records(mates):
    return [len(pack_reads(r, K)[1]) for r in mates]


def same_as_oracle(res, pile, records=None):
    helpers.assert_same_pileup(res, pile)
    n = len(pile.kmc_stats)
    assert res.kmer_stats[:n, 1].tolist() == pile.kmc_stats[:, 1].tolist()        # k-mer occurrences scanned
    assert res.kmer_stats[:, 2].tolist() == [0] * len(res.kmer_stats)              # (the statistics table's: not kept here)
    if records is not None:
        assert res.kmer_stats[:n, 0].tolist() == list(records)                       # records counted (on the host or by K0)


def all_zero(res):
    for a in res.arrays():
        assert not a.any()
    assert not res.stats.any() and not res.present.any() and not res.kmer_stats.any()


def same_results(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.present, b.present) and np.array_equal(a.kmer_stats, b.kmer_stats)


def three_ways(monkeypatch, make_engines, run, env=None):
    """run(engines) -> list of results, once per way on engines made inside that way; the ways' results must be identical."""
    got = {}
    for name in WAYS:
        with way(name, monkeypatch, env or {}):
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


class Sample:
    """reads of one sample (a list of mate files), its oracle pileup and the records its mate files pack to"""

    def __init__(self, oracle, ix, mates):
        self.mates = mates
        self.pile = oracle.sample_pileup(ix, mates)
        self.records = n_records(mates)

    def check(self, res):
        same_as_oracle(res, self.pile, self.records)


@pytest.fixture(scope="module")
def samples(oracle, hpv_ix, hpv_genome):
    """Three samples of different genomes (other variant sites), sizes and error rates, shared by the cases below: a, b of one mate
    file, m of two."""
    a = helpers.hpv_reads(20000, seed=511, err=0.02)
    b = helpers.hpv_reads(6000, seed=512, with_n=True, ragged=True)
    gm, isnv = synth.sample_genome(hpv_genome, 19)
    c1, c2 = synth.paired_codes(gm, 5000, 150, 513, isnv=isnv)
    out = {"a": Sample(oracle, hpv_ix, [a]), "b": Sample(oracle, hpv_ix, [b]),
           "m": Sample(oracle, hpv_ix, [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)])}
    assert int(out["a"].pile.fwd_depth.max()) > 50
    assert len({int(s.pile.kmc_stats[0, 1]) for s in out.values()}) == 3
    return out


def run_and_check(e, sample, **kw):
    res = helpers.hip_sample(e, sample.mates, K, **kw)
    sample.check(res)
    return res


def test_smallest_samples(oracle, hpv_ix, monkeypatch):
    """1, 64 and 65 reads of three different samples, and the first again: one scan workgroup, Level 2's own workgroups and the E bins
    nearly all idle, and behind them the ride, which zeroes what the larger sample before left."""
    sets = [Sample(oracle, hpv_ix, [helpers.hpv_reads(n, seed=500 + n, err=0.02)]) for n in (1, 64, 65)]
    order = [sets[0], sets[1], sets[2], sets[0]]
    assert sets[0].pile.kmc_stats[0, 1] == 130

    def run(engs):
        return [run_and_check(engs[0], s) for s in order]

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


@pytest.mark.parametrize("launches", [1, 2, 4])
def test_the_ride_is_in_the_first_launch_only(samples, hpv_ix, monkeypatch, launches):
    """20,000 reads at 2 % errors as one, two and four scan launches of one push (BK_MAX_LAUNCH_RECORDS, testing library): the ride is in
    the first Level 2 launch; the later ones carry none and wipe nothing.  Between them smaller samples, and one of two mate files."""
    env = {"BK_MAX_LAUNCH_RECORDS": str((20000 + launches - 1) // launches)} if launches > 1 else {}
    order = [samples[c] for c in "abamab"]

    def run(engs):
        return [run_and_check(engs[0], s) for s in order]

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run, env)


@pytest.mark.parametrize("form", ["no push", "shorter than k", "finalize alone"])
def test_a_sample_without_a_level2_launch(samples, hpv_ix, monkeypatch, form):
    """Between two ordinary samples one that launches no Level 2 kernel: nothing pushed (twice in a row: the second follows a sample
    that paid at its finalize), reads all shorter than k, and begin -> finalize -> download on an engine whose previous sample left a
    full pileup.  Its outputs are all zero -- zeroed at the finalize -- and the sample behind it is right."""
    short = [b"ACGT" * 5, b"A" * 20, b"", b"ACGTN" * 4]

    def empty(e):
        e.sample_begin()
        if form == "shorter than k":
            e.push_reads(0, *pack_reads(short, K))
            e.push_reads_ascii(0, short)
        if form == "finalize alone":
            e.sample_finalize(1)
            return e.sample_download(1)
        return e.sample_finish(1)

    def run(engs):
        e = engs[0]
        out = [run_and_check(e, samples["a"]), empty(e)]
        if form == "no push":
            out.append(empty(e))
        out += [run_and_check(e, samples["b"]), empty(e), run_and_check(e, samples["m"]), run_and_check(e, samples["a"])]
        for res in out:
            if int(res.kmer_stats[0, 1]) == 0:
                all_zero(res)
        assert sum(1 for res in out if int(res.kmer_stats[0, 1]) == 0) == (3 if form == "no push" else 2)
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_an_abandoned_sample(samples, hpv_ix, monkeypatch):
    """A sample begun, pushed and begun again (its ride ran, its finalize never did), and one begun and begun again with nothing
    pushed (its zeros still owed): the sample behind each is its own."""
    def run(engs):
        e = engs[0]
        out = [run_and_check(e, samples["a"])]
        e.sample_begin()
        e.push_reads(0, *pack_reads(samples["a"].mates[0], K))
        out.append(run_and_check(e, samples["b"]))
        e.sample_begin()
        out.append(run_and_check(e, samples["m"]))
        e.sample_begin()
        e.push_reads(0, *pack_reads(samples["m"].mates[0], K))
        e.sample_begin()
        e.sample_begin()
        out += [run_and_check(e, samples["b"]), run_and_check(e, samples["a"])]
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def test_two_mate_files_then_one(samples, hpv_ix, monkeypatch):
    """Two mate files, each pushed in two batches: the second mate file's pushes zero nothing of what the first left.  Then a sample of
    one mate file downloaded as two: the second mate file's rows read zero, not what the sample before left there."""
    def run(engs):
        e = engs[0]
        out = [run_and_check(e, samples["b"]), run_and_check(e, samples["m"], batch=3000)]
        e.sample_begin()
        e.push_reads(0, *pack_reads(samples["a"].mates[0], K))
        e.sample_finalize(1)
        res = e.sample_download(2)
        for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk"):
            assert np.array_equal(getattr(res, name), getattr(samples["a"].pile, name)), name
        assert np.array_equal(res.stats[0], samples["a"].pile.stats[0]) and np.array_equal(res.present[0], samples["a"].pile.present[0])
        assert res.kmer_stats[0, :2].tolist() == [samples["a"].records[0], int(samples["a"].pile.kmc_stats[0, 1])]
        assert not res.stats[1].any() and not res.present[1].any() and not res.kmer_stats[1].any()
        out += [res, run_and_check(e, samples["m"]), run_and_check(e, samples["b"])]
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix)], run)


def ascii_device_sample(e, mates):
    """one sample through bk_push_reads_ascii_device, every mate file in two batches"""
    import torch
    e.sample_begin()
    keep = []
    for m, reads in enumerate(mates):
        flat = np.frombuffer(b"".join(reads), np.uint8)
        off = np.zeros(len(reads) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        d_b = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda:0")
        d_b[:len(flat)] = torch.from_numpy(flat.copy()).to("cuda:0")
        cut = [0, len(reads) // 2, len(reads)]
        for a, b in zip(cut, cut[1:]):
            d_off = torch.from_numpy(off[a:b + 1].copy()).to("cuda:0")
            torch.cuda.synchronize()
            e.push_reads_ascii_device(m, d_b.data_ptr(), d_off.data_ptr(), b - a, int(off[b] - off[a]), int((off[a + 1:b + 1] - off[a:b]).max()))
            keep.append(d_off)
        keep.append(d_b)
    res = e.sample_finish(len(mates))
    del keep
    return res


@pytest.mark.parametrize("state", ["plain", "primers", "adapter"])
def test_the_ascii_path_counts_its_records_in_the_samples_own_set(oracle, samples, hpv_ix, hpv_genome, monkeypatch, state):
    """bk_push_reads_ascii_device: K0 (with primers or an adapter set, its *_ends_kernel variants and the trimming kernels behind it)
    adds the records it makes to the k-mer tallies of the sample's parity.  With primers the results are the oracle's on the reads
    with the primer letters written as N, with an adapter on the truncated reads (tests/primer_ref.py, tests/adapter_ref.py)."""
    truseq = adapter_ref.PRESETS["truseq"]
    sets = []
    for seed in (61, 62, 63):
        gm, _ = synth.sample_genome(hpv_genome, seed)
        amps = primer_ref.tile_amplicons(hpv_genome, 60)
        primers = [p for a in amps for p in a[2:]]
        n = 1500 + 400 * (seed - 61)
        if state == "adapter":
            reads = adapter_ref.library_reads(gm, amps, [truseq], n, 150, seed + 1)
            want = adapter_ref.seen_reads(reads, [b"I" * len(r) for r in reads], [truseq], 5, 0.1, K, 0)[0]
        elif state == "primers":
            reads = primer_ref.amplicon_reads(hpv_genome, gm, amps, n, 150, seed + 1)
            want = primer_ref.trimmed(reads, primers, 1)
        else:
            reads = want = helpers.hpv_reads(n, seed=seed, err=0.01, with_n=True)
        seen = Sample(oracle, hpv_ix, [want])
        sets.append((reads, seen))
    assert state == "plain" or any(r != w for (reads, seen) in sets for r, w in zip(reads, seen.mates[0]))

    def make():
        e = helpers.engine_from_oracle_index(hpv_ix)
        if state == "primers":
            e.primers_set(primers, 1)
        if state == "adapter":
            e.adapters_set([truseq], 5, 0.1)
        return [e]

    def run(engs):
        out = []
        for reads, seen in sets + sets[:1]:
            res = ascii_device_sample(engs[0], [reads])
            seen.check(res)
            out.append(res)
        return out

    three_ways(monkeypatch, make, run)


def test_a_family_of_four_and_a_late_fork(samples, hpv_ix, monkeypatch):
    """An engine and three forks take samples in turn (l2_plan_kernel is launched in front of Level 2), each its own sequence of three;
    then a fork made after its parent has run three samples -- an odd number: the fork starts from its own first parity -- and the
    parent again."""
    def make():
        eng = helpers.engine_from_oracle_index(hpv_ix)
        return [eng, eng.fork(), eng.fork(), eng.fork()]

    def run(engs):
        out = []
        for turn in range(3):
            for i, e in enumerate(engs):
                out.append(run_and_check(e, samples["abm"[(turn + i) % 3]]))
        late = engs[0].fork()
        try:
            for c in "mba":
                out += [run_and_check(late, samples[c]), run_and_check(engs[0], samples[c])]
        finally:
            late.close()
        return out

    three_ways(monkeypatch, make, run)


def test_owed_zeros_at_a_sharded_finalize(oracle, samples, hpv_ix, monkeypatch):
    """Two engines stand for two ranks (helpers.sharded_finalize_on_one_device).  After an ordinary sample each, a sample all of whose
    reads rank 0 scanned: rank 1 has pushed nothing, launched no Level 2 kernel, and its zeros are still owed when
    bk_sample_finalize_shard maps its part into its pileup.  Then a sample both scanned half of, and an ordinary one again."""
    def sharded(engs, sample, split):
        words, lens = pack_reads(sample.mates[0], K)
        for e in engs:
            e.sample_begin()
        engs[0].push_reads(0, words[:split], lens[:split])
        engs[1].push_reads(0, words[split:], lens[split:])
        helpers.sharded_finalize_on_one_device(engs, 1, 32)
        out = [e.sample_download(1) for e in engs]
        for res in out:
            sample.check(res)
        return out

    def run(engs):
        out = [run_and_check(engs[0], samples["a"]), run_and_check(engs[1], samples["b"])]
        out += sharded(engs, samples["b"], samples["b"].records[0])
        out += sharded(engs, samples["a"], samples["a"].records[0] // 2)
        out += [run_and_check(engs[0], samples["b"]), run_and_check(engs[1], samples["a"])]
        return out

    def make():
        eng = helpers.engine_from_oracle_index(hpv_ix)
        return [eng, eng.fork()]

    three_ways(monkeypatch, make, run)


def test_full_kmer_stats_keeps_its_launch(oracle, hpv_ix, hpv_genome, monkeypatch):
    """An engine with the statistics table is not eligible (zero_small_kernel zeroes the table's results): three samples, outputs as ever."""
    from bronko_amd import Params
    sets = []
    for seed in (71, 72, 73):
        gm, isnv = synth.sample_genome(hpv_genome, seed)
        c1, c2 = synth.paired_codes(gm, 2000 + 500 * (seed - 71), 150, seed, err=0.01, isnv=isnv)
        mates = [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]
        sets.append((mates, oracle.sample_pileup(hpv_ix, mates)))

    def run(engs):
        out = []
        for mates, pile in sets + sets[:1]:
            res = helpers.hip_sample(engs[0], mates, K)
            helpers.assert_same_pileup(res, pile)
            assert res.kmer_stats[:, 1:4].tolist() == pile.kmc_stats[:, 1:4].tolist()
            out.append(res)
        return out

    three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(hpv_ix, Params(full_kmer_stats=True, kmer_table_log2=20))], run)


def test_four_genomes(oracle, sars_paths, monkeypatch):
    """A four-genome index (nbatch_kernel in front of Level 2, no waiting V items, statistics and presence flags of four files): three
    samples of different genomes of the four."""
    ix = oracle.Index.build(K, sars_paths)
    sets = []
    for g in (2, 0, 3):
        gm, isnv = synth.sample_genome(synth.read_fasta_bytes(sars_paths[g]), 3 + g)
        c1, c2 = synth.paired_codes(gm, 3000 + 500 * g, 150, 80 + g, isnv=isnv)
        sets.append(Sample(oracle, ix, [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]))

    def run(engs):
        return [run_and_check(engs[0], s) for s in sets + sets[:1]]

    try:
        three_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()
