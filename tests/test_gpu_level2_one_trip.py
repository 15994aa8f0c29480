"""level2_kernel finds its marked records in one trip to memory per wave: the working waves share l2_any in stretches of
consecutive words, one word per lane and one load per stretch, and walk only the 64-record steps that hold a mark.  Integer
work: every case equals the CPU oracle bit for bit (HPV16 or SARS-CoV-2, k = 21), on an engine alone and in a family of four,
where the planned grid (l2_plan_kernel) decides how many waves share the words, and three ways that must agree: the release
library, the testing library, the testing library with BK_NO_L2_PLAN=1."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bronko_amd import synth
from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAYS = ("release", "testing", "testing BK_NO_L2_PLAN=1")
COUNTS = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049)   # a word of l2_any, a step of two words, a stretch of 64 words


@contextlib.contextmanager
def way(name, monkeypatch, env):
    """Engines created inside bind the library `name` says; `env`: testing aids (the release library reads none)."""
    from bronko_amd import _ffi
    _ffi.use_testing_library(name != "release")
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    if name.endswith("BK_NO_L2_PLAN=1"):
        monkeypatch.setenv("BK_NO_L2_PLAN", "1")
    try:
        yield
    finally:
        for key in list(env) + ["BK_NO_L2_PLAN"]:
            monkeypatch.delenv(key, raising=False)
        _ffi.use_testing_library(False)


def same_as_oracle(res, pile):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[:len(pile.kmc_stats), 1].tolist() == pile.kmc_stats[:, 1].tolist()    # k-mer occurrences scanned


def same_results(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.present, b.present) and np.array_equal(a.kmer_stats, b.kmer_stats)


def packed(reads):
    from bronko_amd import pack_reads
    return pack_reads(reads, 21)


def sample(eng, pk, batch=None):
    """One single-file sample of reads packed once (helpers.hip_sample packs them at every call)."""
    words, lens = pk
    eng.sample_begin()
    for i in range(0, len(lens), batch or max(len(lens), 1)):
        eng.push_reads(0, words[i:i + (batch or len(lens))], lens[i:i + (batch or len(lens))])
    return eng.sample_finish(1)


def every_way(monkeypatch, ix, run, env=None):
    """run(engine) -> list of results, checked against the oracle inside.  Per way: on a new engine alone, then on that engine and on
    one of three forks of it (a family of four).  All six lists must be identical."""
    got = []
    for name in WAYS:
        with way(name, monkeypatch, env or {}):
            eng = helpers.engine_from_oracle_index(ix)
            forks = []
            try:
                got.append(run(eng))
                forks = [eng.fork(), eng.fork(), eng.fork()]
                got.append(run(eng))
                got.append(run(forks[1]))
            finally:
                for e in forks + [eng]:
                    e.close()
    for other in got[1:]:
        assert len(other) == len(got[0])
        for a, b in zip(got[0], other):
            same_results(a, b)


@pytest.fixture(scope="module")
def hpv_ix(oracle, golden_dir):
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def hpv_genome():
    return synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))


def reference_reads(genome, n, seed):
    """Reads of the reference itself, without an error: the scan settles them all and marks nothing."""
    return synth.codes_to_ascii(synth.single_end_codes(genome, n, 150, seed, err=0.0))


def test_word_step_and_stretch_boundaries_nearly_every_record_marked(oracle, hpv_ix, monkeypatch):
    """1 .. 2049 reads at 5 % errors: nearly every record is marked, up to and one beyond a word, a step and a 64-word stretch."""
    reads = helpers.hpv_reads(COUNTS[-1], seed=401, err=0.05)
    piles = [oracle.sample_pileup(hpv_ix, [reads[:n]]) for n in COUNTS]

    def run(eng):
        out = [helpers.hip_sample(eng, [reads[:n]], 21) for n in COUNTS]
        for res, pile in zip(out, piles):
            same_as_oracle(res, pile)
        return out

    every_way(monkeypatch, hpv_ix, run)


def test_word_step_and_stretch_boundaries_only_the_last_record_marked(oracle, hpv_ix, hpv_genome, monkeypatch):
    """The same counts of error-free reads of the reference, the last one replaced by a read with 5 % errors: one mark, in the
    launch's last word -- every step in front of it is skipped."""
    clean = reference_reads(hpv_genome, COUNTS[-1], 402)
    noisy = helpers.hpv_reads(len(COUNTS), seed=403, err=0.05)
    sets = [clean[:n - 1] + [noisy[i]] for i, n in enumerate(COUNTS)]
    piles = [oracle.sample_pileup(hpv_ix, [s]) for s in sets]

    def run(eng):
        out = [helpers.hip_sample(eng, [s], 21) for s in sets]
        for res, pile in zip(out, piles):
            same_as_oracle(res, pile)
        return out

    every_way(monkeypatch, hpv_ix, run)


def test_a_wave_goes_round_three_times(oracle, hpv_ix, hpv_genome, monkeypatch):
    """A launch of more stretches than working waves.  Level 2's working grid is never below ScanArgs::l2_min_grid (half the CUs:
    a million records a round), so the testing library's BK_L2_MIN_GRID=1 lowers the floor: 40,000 records with one read in a
    hundred at 5 % errors are 400 marked records -> two workgroups, eight waves, twenty stretches of 64 words; with the last
    record alone marked one workgroup, whose four waves take five stretches each.  BK_ITEM_GRID=3 on top: the marks come from three
    scan workgroups.  (The release library and BK_NO_L2_PLAN=1 run the same reads on their own grids.)"""
    clean = reference_reads(hpv_genome, 40000, 411)
    noisy = helpers.hpv_reads(400, seed=412, err=0.05)
    sparse = list(clean)
    sparse[99::100] = noisy
    last = clean[:-1] + [noisy[0]]
    p_sparse, p_last = oracle.sample_pileup(hpv_ix, [sparse]), oracle.sample_pileup(hpv_ix, [last])
    k_sparse, k_last = packed(sparse), packed(last)

    def run(eng):
        out = [sample(eng, k_sparse), sample(eng, k_last), sample(eng, k_sparse, batch=25000)]
        for res, pile in zip(out, (p_sparse, p_last, p_sparse)):
            same_as_oracle(res, pile)
        return out

    every_way(monkeypatch, hpv_ix, run, {"BK_L2_MIN_GRID": "1", "BK_ITEM_GRID": "3"})


def test_the_plan_above_its_floor(oracle, sars_paths, monkeypatch):
    """40,000 SARS-CoV-2 reads at 5 % errors: more than 256 x 128 = 32,768 marked records, the plan above its floor."""
    ix = oracle.Index.build(21, sars_paths[:1])
    gm, isnv = synth.sample_genome(synth.read_fasta_bytes(sars_paths[0]), 5)
    reads = synth.codes_to_ascii(synth.single_end_codes(gm, 40000, 150, 421, err=0.05, isnv=isnv))
    pile = oracle.sample_pileup(ix, [reads])
    pk = packed(reads)

    def run(eng):
        out = [sample(eng, pk)]
        same_as_oracle(out[0], pile)
        return out

    try:
        every_way(monkeypatch, ix, run)
    finally:
        ix.close()


def test_a_small_launch_after_a_large_one(oracle, hpv_ix, monkeypatch):
    """20,000 reads and then 70 as two launches of one sample, and again as the next sample: a launch of three words of l2_any
    behind one of 625, whose words beyond the third must all be zero again."""
    reads = helpers.hpv_reads(20070, seed=431, err=0.05)
    pile = oracle.sample_pileup(hpv_ix, [reads])
    pk = packed(reads)

    def run(eng):
        out = [sample(eng, pk, batch=20000), sample(eng, pk, batch=20000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    every_way(monkeypatch, hpv_ix, run)


def test_an_abandoned_sample_leaves_no_mark(oracle, hpv_ix, hpv_genome, monkeypatch):
    """A sample of 5 % errors begun, pushed and abandoned, then an error-free one: a mark left behind would be looked at again."""
    from bronko_amd import pack_reads
    noisy = helpers.hpv_reads(6000, seed=441, err=0.05)
    clean = reference_reads(hpv_genome, 6000, 442)
    p_clean, p_noisy = oracle.sample_pileup(hpv_ix, [clean]), oracle.sample_pileup(hpv_ix, [noisy])

    def run(eng):
        eng.sample_begin()
        eng.push_reads(0, *pack_reads(noisy, 21))
        out = [helpers.hip_sample(eng, [clean], 21), helpers.hip_sample(eng, [noisy], 21)]
        same_as_oracle(out[0], p_clean)
        same_as_oracle(out[1], p_noisy)
        return out

    every_way(monkeypatch, hpv_ix, run)


def test_two_sequences_and_their_n_runs(oracle, hpv_genome, monkeypatch):
    """HPV16 cut into two sequences of one file: reads across the cut are N runs, nbatch_kernel (which keeps its own walk over its
    own marks) marks for Level 2 after the scan, and the discovery finds the marks of both."""
    ix = oracle.Index.build_mem(21, [("two", [("front", hpv_genome[:4100]), ("back", hpv_genome[4100:])])])
    reads = helpers.hpv_reads(12000, seed=451, err=0.02)
    pile = oracle.sample_pileup(ix, [reads])
    pk = packed(reads)

    def run(eng):
        out = [sample(eng, pk), sample(eng, pk, batch=5000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        every_way(monkeypatch, ix, run)
    finally:
        ix.close()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from bronko_amd import Params, _ffi, pack_reads, synth
from bronko_amd.hostlib import HostIndex
from tests import helpers
_ffi.use_testing_library(True)
g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
clean = synth.codes_to_ascii(synth.single_end_codes(g, 20000, 150, 461, err=0.0))
noisy = helpers.hpv_reads(20000, seed=462, err=0.05)
some = list(clean[:5000]); some[::4] = noisy[:1250]
eng = HostIndex.load(os.path.join(helpers.GOLDEN, "hpv.bkdb")).engine(Params(device=0))
forks = [eng.fork(), eng.fork(), eng.fork()]
for name, reads, batch in (("noisy", noisy, None), ("last", clean[:-1] + noisy[:1], None), ("some", some, None), ("two launches", noisy, 12000)):
    sys.stderr.write("[case] %%s\n" %% name); sys.stderr.flush()
    helpers.hip_sample(eng, [reads], 21, batch=batch)
for e in forks + [eng]:
    e.close()
"""


def test_tallies_of_the_scan_and_the_discovery_agree():
    """BK_L2_STATS=1 in a child process (the testing library prints its tallies on stderr at every finalize), a family of four with
    BK_L2_MIN_GRID=2: the records the scan counted as newly marked are the records the discovery queued, and the working grid is
    min(Level 2's grid, max(2, ceil(marked / 256))) -- the whole grid of 20 workgroups for 20,000 reads at 5 % errors (three in four
    are marked: a read whose errors all lie k bases apart is settled by the scan), the floor for a single mark, between the two
    for 1,250 such reads among 5,000 error-free ones (a grid of 5).  An error-free read of the reference is never marked."""
    env = dict(os.environ, BK_L2_STATS="1", BK_L2_MIN_GRID="2")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got, case = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            case = line[7:]
        m = re.match(r"\[bk\] level 2 discovery: (\d+) records newly marked by the scan, (\d+) records queued, g_work (\d+)", line)
        if m:
            got[case] = tuple(int(x) for x in m.groups())
    assert sorted(got) == ["last", "noisy", "some", "two launches"], r.stderr[-4000:]
    for case, (new, queued, g_work) in got.items():
        print(case, new, queued, g_work)
        assert new == queued, case
    assert 0 < got["noisy"][0] <= 20000 and got["two launches"][0] == got["noisy"][0]
    assert got["last"][0] == 1 and 0 < got["some"][0] <= 1250
    for case, n_records in (("noisy", 20000), ("last", 20000), ("some", 5000), ("two launches", 8000)):
        n_l2 = ((n_records + 255) // 256 + 3) // 4
        marked = got[case][0] if case != "two launches" else None
        if marked is not None:
            assert got[case][2] == min(n_l2, max(2, (marked + 255) // 256)), case
        else:
            assert 2 <= got[case][2] <= n_l2, case
