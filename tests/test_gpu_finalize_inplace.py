"""The regional finalize settles its items in place (finalize_vbin_kernel, bk_finalize_lean.hip): a V k-mer that is not "one
BucketInfo, known from the record" and a reference k-mer that is not simple go on the workgroup's own list in LDS, the workgroup's
waves walk the list's items' buckets behind the row loop, an item that finds the list full is settled where it was found, and the
workgroup zeroes the E counters it read.  No finalize_general_kernel, no list in device memory.

Integer work: every case equals the CPU oracle bit for bit -- four pileup arrays, statistics, presence flags, the k-mers scanned --
and runs three ways that must agree in everything, the distinct / kept k-mer tallies included: the release library, the testing
library, and the testing library with BK_NO_LEAN_FINALIZE=1 (the general finalize, which shares no code with the list).  (Without a
statistics table the engine's distinct / kept tallies count the k-mers that touch the index only, which the oracle does not report:
the general finalize is their reference.)  The shapes are the smallest at which the list can go wrong: items of both kinds in one
workgroup, a list of one and of three entries under a region of repeats, thresholds that bite on a repeat's counters, samples
behind one another on planes the workgroups have to leave clean, a workgroup of rows only, rows of 15 and of 25 counters, four
engines' workgroups on the same CUs, two mate files."""
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
WAYS = ("release", "testing", "testing BK_NO_LEAN_FINALIZE=1")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LIST_CAP = 256   # kLeanListCap (bk_kernels.h)


@contextlib.contextmanager
def way(name, monkeypatch):
    """Engines created inside bind the library `name` says; NAME=VALUE (or NAME: 1) behind it is set in the environment meanwhile."""
    from bronko_amd import _ffi
    _ffi.use_testing_library(name != "release")
    env = [(w.split("=") + ["1"])[:2] for w in name.split()[1:]]
    for var, val in env:
        monkeypatch.setenv(var, val)
    try:
        yield
    finally:
        for var, _ in env:
            monkeypatch.delenv(var, raising=False)
        _ffi.use_testing_library(False)


def same_as_oracle(res, pile):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[:len(pile.kmc_stats), 1].tolist() == pile.kmc_stats[:, 1].tolist()    # k-mer occurrences scanned


def same_results(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.present, b.present)
    assert np.array_equal(a.kmer_stats, b.kmer_stats), (a.kmer_stats, b.kmer_stats)            # (distinct / kept among them)


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
    """finalize_runs_by_region's conditions on the index, restated (bk_device.h v_layout_span): one genome file of one sequence with
    dense planes and default parameters is given; what is left is a window of more than one bucket, no pseudo k-mers and rows of at
    most 32 counters.  Returns the rows a wave takes per pass, or 0."""
    wstart, W = n_fixed, k - 2 * n_fixed - 1
    omin = min(wstart, k - wstart - W)
    span = max(wstart + W - 1, k - 1 - wstart) - omin + 1
    return 64 // span if (W > 1 and k < 31 and 0 < span <= 32) else 0


def random_reference(n, seed):
    return synth.codes_to_ascii(np.ascontiguousarray((synth.splitmix64(seed, n) >> np.uint64(33)).astype(np.uint8).reshape(1, n) & 3))[0]


def canonical_kmers(seq, k):
    out = []
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        rc = w.translate(COMP)[::-1]
        out.append((min(w, rc), rc < w))
    return out


def reads_of(ref, n, read_len, seed, err=0.02):
    return synth.codes_to_ascii(synth.single_end_codes(ref, n, read_len, seed, err=err))


def crafted_reference():
    """The 559 bp of test_gpu_finalize_lean_staged.py::test_repeats_and_near_repeats_across_a_region_boundary: a stretch S of 64 bp
    three times, the third reverse-complemented (ids that are not simple: E items), its first copy on both sides of the boundary
    between the first two regions, and a stretch T of 50 bp again with one and with two substitutions (dirty ids whose answers say
    "several" or "none": V items) -- both kinds of item in one workgroup."""
    rnd = random_reference(400, 4130)
    S, T = rnd[0:64], rnd[64:114]
    T1 = bytearray(T); T1[25] = ord("A") if T1[25] != ord("A") else ord("C"); T1 = bytes(T1)
    T2 = bytearray(T1); T2[31] = ord("G") if T2[31] != ord("G") else ord("T"); T2 = bytes(T2)
    ref = rnd[120:160] + S + rnd[160:190] + T + rnd[190:215] + S + rnd[215:245] + T1 + rnd[245:275] + S.translate(COMP)[::-1] + rnd[275:300] + T2 + rnd[300:337]
    assert len(ref) == 559 and ref[40:104] == S
    return ref


def repeated_reference():
    """One stretch of 64 bp nine times and 24 bp more of it, 600 bp, with one base of the fifth copy changed: the 64 k-mers of the
    stretch's circle are the ids of the whole first region, every one a repeat (not simple), and a k-mer one base from one of them
    neighbours a repeat: nearly every counter there is an item.  (The densest such reference the regional finalize accepts: without
    the changed base no reference k-mer is within two bases of another, no answer table is built, and finalize_lean_ok turns the
    index away -- the 21 k-mers over the changed base, ids 64 ... 84, are the dirty ones that make it.)"""
    unit = random_reference(64, 4160)
    ref = bytearray((unit * 10)[:600])
    ref[300] = ord("A") if ref[300] != ord("A") else ord("C")
    return bytes(ref)


def short_reference_with_a_duplicate():
    """The 70 bp of test_reference_shorter_than_one_region with its bases 5 ... 34 again at 38 ... 67: fewer reference k-mers than
    one region has ids, the duplicated stretch's k-mers are not simple, and the second workgroup owns rows only -- V items, no ids."""
    ref = bytearray(random_reference(70, 4101))
    ref[38:68] = ref[5:35]
    return bytes(ref)


@pytest.fixture(scope="module")
def crafted(oracle):
    """The crafted reference's index at k = 21, 6,000 reads of 100 bp and their oracle pileup, computed once."""
    ref = crafted_reference()
    assert regional_finalize_applies(21) == 3
    ix = oracle.Index.build_mem(21, [("crafted", [("ref", ref)])])
    reads = reads_of(ref, 6000, 100, 4131)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_depth[(40 + 30) * 4:(40 + 30) * 4 + 4].max()) > 20
    yield ref, ix, reads, pile
    ix.close()


# ---- the samples' item tallies, from one child process with BK_L2_STATS (the testing library prints them at every finalize) --------
CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from bronko_amd import _ffi
from oracle import oracle as orc
from tests import helpers
from tests import test_gpu_finalize_inplace as t
_ffi.use_testing_library(True)
orc.build()
for name, ref, n_reads, read_len, seed in (("crafted", t.crafted_reference(), 6000, 100, 4131), ("repeated", t.repeated_reference(), 3000, 100, 4161),
                                           ("short", t.short_reference_with_a_duplicate(), 600, 50, 4102)):
    ix = orc.Index.build_mem(21, [(name, [("ref", ref)])])
    reads = t.reads_of(ref, n_reads, read_len, seed)
    eng = helpers.engine_from_oracle_index(ix)
    for batch in (None, (n_reads + 1) // 2):
        sys.stderr.write("[case] %%s %%s\n" %% (name, "items" if batch is None else "plane")); sys.stderr.flush()
        helpers.hip_sample(eng, [reads], 21, batch=batch)
    eng.close(); ix.close()
"""


@pytest.fixture(scope="module")
def tallies():
    """{"<reference> <items | plane>": items of the sample (V and E items alike)}."""
    env = dict(os.environ, BK_L2_STATS="1")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got, case = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            case = line[7:]
        m = re.match(r"\[bk\] finalize: (\d+) \+ (\d+) k-mers deferred", line)
        if m:
            got[case] = int(m.group(1)) + int(m.group(2))
    assert sorted(got) == sorted("%s %s" % (a, b) for a in ("crafted", "repeated", "short") for b in ("items", "plane")), r.stderr[-4000:]
    print(got)
    return got


def test_items_of_both_kinds_in_one_workgroup(crafted, tallies, monkeypatch):
    """The crafted reference, 6,000 reads of 100 bp, as one launch (the items' instantiation) and as two (the plane's): S's first copy
    puts E items, T's neighbours V items on the lists of the first two workgroups.  The child's tallies say the path was taken."""
    ref, ix, reads, pile = crafted
    assert tallies["crafted items"] > 0 and tallies["crafted plane"] == tallies["crafted items"]

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], 21), helpers.hip_sample(engs[0], [reads], 21, batch=3000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)


@pytest.mark.parametrize("cap", [1, 3, None])
def test_a_full_list(oracle, tallies, monkeypatch, cap):
    """600 bp that are one stretch of 64 bp over and over: every id of the first region is a repeat and nearly every V k-mer an item.  With
    BK_LEAN_LIST_CAP at 1 and at 3 all but one or three of a workgroup's items are settled by the wave that found them; at the
    default the busiest workgroups' lists still run full.  The sample has more items than the list has entries."""
    ref = repeated_reference()
    km = canonical_kmers(ref, 21)
    assert len(ref) == 600 and len({c for c, _ in km}) == 64 + 21 and len({c for c, _ in km[:64]}) == 64 and regional_finalize_applies(21)
    assert all(sum(1 for c2, _ in km if c2 == c) >= 8 for c, _ in km[:64])       # (the first region's ids: every one a repeat)
    assert tallies["repeated items"] > (cap or LIST_CAP) and tallies["repeated plane"] == tallies["repeated items"]
    ix = oracle.Index.build_mem(21, [("repeated", [("ref", ref)])])
    reads = reads_of(ref, 3000, 100, 4161)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_depth.max()) > 0 and int(pile.rev_depth.max()) > 0

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], 21), helpers.hip_sample(engs[0], [reads], 21, batch=1500)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    testing = "testing" if cap is None else "testing BK_LEAN_LIST_CAP=%d" % cap
    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run, ("release", testing, "testing BK_NO_LEAN_FINALIZE=1"))
    finally:
        ix.close()


def test_thresholds_on_listed_ids(oracle, crafted, monkeypatch):
    """ci = 2 and cs = 40 on the crafted reference: a repeat's E counter holds the reads of three copies and saturates, a counter of 1
    is dropped by the thread that lists the id -- its distinct / kept tallies are the ones finalize_general_kernel kept."""
    from bronko_amd import Params
    ref, ix, reads, pa = crafted
    assert int(max(pa.fwd_depth.max(), pa.rev_depth.max())) > 40
    pile = oracle.sample_pileup(ix, [reads], ci=2, cs=40)
    s_cells = slice((40 + 21) * 4, (40 + 43) * 4)                                # inside S's first copy
    assert int(max(pile.fwd_depth[s_cells].max(), pile.rev_depth[s_cells].max())) == 40
    assert int(pile.fwd_nk.sum()) > int(pa.fwd_nk.sum())                         # (k-mers seen twice count now)

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], 21), helpers.hip_sample(engs[0], [reads], 21, batch=3000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix, Params(ci=2, cs=40))], run)


def test_the_planes_are_clean_behind_the_sample(oracle, crafted, monkeypatch):
    """One engine: the sample with repeats, error-free reads of another part of the reference, the first again -- whatever E counter
    a workgroup did not zero behind the first shows in the second --, then a sample begun, pushed and abandoned in front of both."""
    from bronko_amd import pack_reads
    ref, ix, reads, pile = crafted
    clean = reads_of(ref[447:], 1500, 60, 4171, err=0.0)                        # (behind the last copy of S: T2 and what surrounds it)
    pc = oracle.sample_pileup(ix, [clean])
    assert int(pc.fwd_nk[:134 * 4].sum() + pc.rev_nk[:134 * 4].sum()) == 0 and int(pc.fwd_nk.sum()) > 0   # (nothing of it in front of T)

    def run(engs):
        e = engs[0]
        out = [helpers.hip_sample(e, [reads], 21), helpers.hip_sample(e, [clean], 21), helpers.hip_sample(e, [reads], 21, batch=3000),
               helpers.hip_sample(e, [clean], 21, batch=750)]
        e.sample_begin()                       # abandoned: its counters are still in the plane
        e.push_reads(0, *pack_reads(reads, 21))
        out += [helpers.hip_sample(e, [clean], 21), helpers.hip_sample(e, [reads], 21)]
        for res, p in zip(out, (pile, pc, pile, pc, pc, pile)):
            same_as_oracle(res, p)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)


def test_a_workgroup_of_rows_only(oracle, tallies, monkeypatch):
    """70 bp with 30 of them twice: 50 - 10 reference k-mers, n_full < 64; the first workgroup has ids and rows, the second rows only --
    its items are V items, its id_lo is clamped, the K2e part meets nothing but ids past n_full."""
    ref = short_reference_with_a_duplicate()
    km = canonical_kmers(ref, 21)
    assert len({c for c, _ in km}) == 40 and km[5][0] == km[38][0]
    assert tallies["short items"] > 0 and tallies["short plane"] == tallies["short items"]
    ix = oracle.Index.build_mem(21, [("short", [("ref", ref)])])
    reads = reads_of(ref, 600, 50, 4102)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_depth.max()) > 0 and int(pile.rev_depth.max()) > 0

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], 21), helpers.hip_sample(engs[0], [reads], 21, batch=300)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


@pytest.mark.parametrize("k", [19, 29])
def test_other_row_shapes(oracle, monkeypatch, k):
    """The crafted reference at k = 19 (rows of 15 counters, four per wave) and k = 29 (rows of 25, two per wave): lists fed from
    other shapes of the row loop, windows of 14 and 24 buckets walked by the lanes."""
    assert regional_finalize_applies(k) == {19: 4, 29: 2}[k]
    ref = crafted_reference()
    ix = oracle.Index.build_mem(k, [("crafted", [("ref", ref)])])
    reads = reads_of(ref, 6000, 100, 4180 + k)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_depth.max()) > 20

    def run(engs):
        out = [helpers.hip_sample(engs[0], [reads], k), helpers.hip_sample(engs[0], [reads], k, batch=3000)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    try:
        all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
    finally:
        ix.close()


def test_four_engines_in_turn(crafted, monkeypatch):
    """An engine and three forks run the crafted sample on their own streams, all begun before any is finalized, twice: four
    samples' workgroups with lists share CUs, and every engine's planes are clean for its second turn."""
    from bronko_amd import pack_reads
    ref, ix, reads, pile = crafted
    words, lens = pack_reads(reads, 21)

    def make():
        eng = helpers.engine_from_oracle_index(ix)
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
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, make, run)


def test_two_mate_files(oracle, crafted, monkeypatch):
    """Two mate files of the crafted reference: two planes, two launches of the kernel into the same pileup, n_deferred per mate."""
    ref, ix, reads, _ = crafted
    c1, c2 = synth.paired_codes(ref, 3000, 100, 4191, err=0.02)
    mates = [synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)]
    pile = oracle.sample_pileup(ix, mates)
    assert int(pile.fwd_depth.max()) > 20

    def run(engs):
        out = [helpers.hip_sample(engs[0], mates, 21), helpers.hip_sample(engs[0], mates, 21, batch=1500)]
        for res in out:
            same_as_oracle(res, pile)
        return out

    all_ways(monkeypatch, lambda: [helpers.engine_from_oracle_index(ix)], run)
