"""bk_copybacks_enable / bk_sample_copybacks (bk_copybacks.hip) against the Python restatement of the rule (tests/copybacks_ref.py):
the whole event table (min_reads 1, min_dist 0), the whole span array and every tally must be equal -- the rule is integer
arithmetic, no case is left out.  Then the C ABI's call order, the feature next to the others, and `bronko call --copybacks` end
to end."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import copyback_cases, copybacks_ref, junction_cases, junctions_ref
from tests.copybacks_ref import H, T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HPV = os.path.join(GOLDEN, "HPV16.fa")
K = 21
SITES = [(1000 + 700 * i, 1350 + 700 * i + 37 * (i % 3), 0) for i in range(8)]   # pairs of HPV16 cells at which the sample's reads gather


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _finish(eng, n_mates=1, min_reads=1, min_dist=0):
    eng.sample_finalize(n_mates)
    eng.sample_copybacks(min_reads, min_dist)
    summ, rows = eng.download_copybacks()
    return summ, rows, eng.download_copyback_span()


def _tallies(summ):
    return (summ.records, summ.same_strand, summ.ref_spanning, summ.switched, summ.supporting, summ.discordant)


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = copybacks_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    assert _tallies(summ) == copybacks_ref.counters_tuple(res), (what, _tallies(summ), res.counters)
    assert summ.candidates == summ.reported == len(res.events) and summ.overflow == 0, what


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _one(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    return _finish(eng)


class World:
    """HPV16 at k = 21: the index, the genome as the restatement sees it, a 2,000-read sample and what the rule makes of it"""

    def __init__(self):
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.g = copybacks_ref.read_fasta(HPV, K)
        self.reads = copyback_cases.sample_reads(self.g.text, SITES, 7, n_reads=2000, switch=0.3)
        self.res = copybacks_ref.copyback_events(self.g, self.reads)
        assert len(self.res.events) >= 100 and all(v > 0 for v in self.res.counters.values())
        assert {key[0] for key, (lf, hf) in self.res.events.items() if lf + hf >= 5} == {H, T}
        self.eng = self.ix.engine()
        self.eng.copybacks_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    """Every crafted case of tests/copyback_cases.py (what each is meant to be: tests/test_copybacks_cpu.py), as it is and
    reverse-complemented"""
    seqs = copyback_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = copybacks_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    cases = copyback_cases.crafted_cases(k)[0]
    reads = [r for _, r, _ in cases]
    eng = ix.engine()
    try:
        for M in (2, 0, 3, 8):
            eng.copybacks_enable(M)
            res = copybacks_ref.copyback_events(g, reads, M)
            assert len(res.events) >= 20 and (res.counters["discordant"] > 0 or M >= 3)
            _check(_one(eng, reads, k), g, res, (k, M))
        eng.copybacks_enable(2)
        for label, read, _ in cases:                               # ... and one by one, so that a difference names its record
            _check(_one(eng, [read], k), g, copybacks_ref.copyback_events(g, [read], 2), label)
    finally:
        eng.close()
        ix.close()


def _switched_reads(w):
    return [r for r in w.reads if copybacks_ref.copyback_events(w.g, [r]).counters["switched"]]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    reads = (_switched_reads(world)[:n // 2 + 1] + world.reads)[:n]
    res = copybacks_ref.copyback_events(world.g, reads)
    assert res.events
    _check(_one(world.eng, reads), world.g, res, n)


@pytest.mark.parametrize("order", ["consecutive", "alternating"])
def test_the_queue_carries_over_drains_at_64_and_walks_a_remainder(world, order):
    """200 switched records one after the other: three waves queue 64 and walk them at once, the fourth walks a remainder of 8.
    Alternating with plain records every wave queues 32 and walks them as a remainder.  (Records that wait from one trip of the
    grid to the next need more records than the grid holds: tests/test_gpu_copyback_trips.py.)"""
    sw = copyback_cases.sample_reads(world.g.text, SITES, 3, n_reads=260, switch=1.0)
    sw = [r for r in sw if copybacks_ref.copyback_events(world.g, [r]).counters["switched"]][:200]
    assert len(sw) == 200
    plain = [r for r in world.reads if copybacks_ref.copyback_events(world.g, [r]).counters["switched"] == 0]
    reads = sw + plain[:56] if order == "consecutive" else [r for pair in zip(sw, plain[:200]) for r in pair]
    res = copybacks_ref.copyback_events(world.g, reads)
    assert res.counters["switched"] == 200 and len(res.events) > 50
    _check(_one(world.eng, reads), world.g, res, order)


def test_the_sample_in_one_push_and_in_several(world):
    for cuts in ([0, len(world.reads)], [0, 37, 700, 1301, len(world.reads)]):
        world.eng.sample_begin()
        for a, b in zip(cuts, cuts[1:]):
            _packed(world.eng, 0, world.reads[a:b])
        _check(_finish(world.eng), world.g, world.res, len(cuts))
    world.eng.sample_begin()
    world.eng.push_reads_ascii(0, _b(world.reads))
    _check(_finish(world.eng), world.g, world.res, "ascii")


def test_two_mate_files_add_into_one_table(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads[:900])
    _packed(eng, 1, world.reads[900:])
    _check(_finish(eng, 2), world.g, world.res)


def test_a_read_and_its_reverse_complement_swap_the_counters(world):
    """A sample and the sample reverse-complemented: the same events and spans, lo_first and hi_first exchanged (a hairpin's two
    cells are one: both orientations count lo_first there, and over a palindrome nothing is asked)"""
    reads = world.reads[:800]
    fwd = _one(world.eng, reads)
    rev = _one(world.eng, [copybacks_ref.revcomp(r) for r in reads])
    assert np.array_equal(fwd[2], rev[2]) and _tallies(fwd[0]) == _tallies(rev[0])
    assert [r[:3] for r in fwd[1]] == [r[:3] for r in rev[1]] and len(fwd[1]) > 50
    plain = [(a, b) for a, b in zip(fwd[1], rev[1]) if copybacks_ref.homology(world.g, a[2], a[0], a[1]) == 0 and a[0] != a[1]]
    assert len(plain) > 20 and all((a[3], a[4]) == (b[4], b[3]) for a, b in plain)


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_copybacks(1)
        assert ei.value.status == -5
        fork.copybacks_enable(2, 12)
        other = copybacks_ref.copyback_events(world.g, world.reads[:500])
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.sample_begin()                                         # an engine that never enabled the pass has nothing of it
        _packed(eng, 0, world.reads[:100])
        eng.sample_finalize(1)
        for fn in (eng.sample_copybacks, eng.download_copybacks, eng.download_copyback_span):
            with pytest.raises(BronkoError) as ei:
                fn()
            assert ei.value.status == -5
        eng.copybacks_enable(2, 14)
        with pytest.raises(BronkoError) as ei:                     # enabled after the last sample began: that sample has no events
            eng.sample_copybacks(1)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        _check(_one(eng, world.reads[:500]), world.g, copybacks_ref.copyback_events(world.g, world.reads[:500]))
        eng.copybacks_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:500])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_copybacks(1)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        eng.copybacks_enable(0, 10)
        res = copybacks_ref.copyback_events(world.g, world.reads[:500], 0)
        assert res.events and res.counters["discordant"] > 0
        _check(_one(eng, world.reads[:500]), world.g, res)
        # a sample that is begun, pushed and never finalized leaves nothing behind
        eng.sample_begin()
        _packed(eng, 0, world.reads[500:1500])
        _check(_one(eng, world.reads[:500]), world.g, res)
    finally:
        eng.close()


def test_a_full_table_is_an_error_not_a_loss(world):
    g = world.g
    reads = [copyback_cases.turn_read(g.text, H if i % 2 else T, 1000 + i, 3000 + 2 * i, 40, 40) for i in range(1500)]   # 1,500 distinct turns
    res = copybacks_ref.copyback_events(g, reads)
    assert len(res.events) > 1024
    eng = world.ix.engine()
    try:
        eng.copybacks_enable(2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_copybacks(1)
        summ = _ffi.CopybackSummary()
        assert eng._L.bk_sample_download_copybacks(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate copy-backs" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_copybacks()
        _check(_one(eng, reads[:800]), g, copybacks_ref.copyback_events(g, reads[:800]))   # the next sample is clean
        eng.copybacks_enable(2, 12)
        _check(_one(eng, reads), g, res)
    finally:
        eng.close()


def test_call_order_and_parameters(world):
    eng = world.ix.engine()

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status

    try:
        for bad in ((9, 16), (2, 9), (2, 25)):
            assert status(eng.copybacks_enable, *bad) == -1
        assert status(eng.sample_copybacks, 1) == -5                  # not enabled
        eng.copybacks_enable()
        assert status(eng.sample_copybacks, 1) == -5                  # nothing was ever begun
        assert status(eng.download_copybacks) == -5 and status(eng.download_copyback_span) == -5
        eng.sample_begin()
        assert status(eng.copybacks_enable) == -5 and status(eng.copybacks_enable, None) == -5   # inside a sample
        assert status(eng.sample_copybacks, 1) == -5
        _packed(eng, 0, world.reads[:1200])
        eng.sample_finalize(1)
        assert status(eng.download_copybacks) == -5                   # finalized, but no report was made
        assert status(eng.sample_copybacks, 0) == -1
        res = copybacks_ref.copyback_events(world.g, world.reads[:1200])
        eng.sample_copybacks(1)                                       # needs the finalize only, not bk_sample_call
        full = eng.download_copybacks()[1]
        assert full == copybacks_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_copybacks(cap=2)                    # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 8), 0xffffffff, np.uint32), _ffi.CopybackSummary()
        assert eng._L.bk_sample_download_copybacks(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert (raw[:2, 7] == 0).all()
        assert eng._L.bk_sample_download_copybacks(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_copybacks(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_copyback_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1
        seen = set()
        most = max(r[3] + r[4] for r in full)
        for min_reads, min_dist in ((most, 0), (most + 1, 0), (2, 0), (1, 1), (1, 400), (2, 400), (1, 1 << 27), (1, 0)):   # again with other thresholds
            eng.sample_copybacks(min_reads, min_dist)
            summ, rows = eng.download_copybacks()
            assert rows == copybacks_ref.table_rows(world.g, res, min_reads, min_dist) and summ.candidates == len(full) and summ.reported == len(rows)
            seen.add(len(rows))
        assert len(seen) >= 6 and 0 in seen
        assert any(r[0] == r[1] for r in full) and len(copybacks_ref.table_rows(world.g, res, 1, 1)) < len(full)   # min_dist 1 drops the hairpins
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_copybacks(1)
        assert eng.download_copybacks()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_copybacks) == -5 and status(eng.sample_copybacks, 1) == -5
        eng.sample_finalize(1)
        eng.sample_copybacks(1)
        summ, rows = eng.download_copybacks()
        assert rows == [] and summ.records == 0 and not eng.download_copyback_span().any()
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.copybacks_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_fuzz_against_the_restatement():
    """tests/copyback_cases.fuzz_world: 2,500 reads of 64 to 150 bases of a random two-sequence genome with planted turn sites, half
    of them strand switches of both kinds with 0 to 4 substitutions"""
    seqs, reads = copyback_cases.fuzz_world()
    g = copybacks_ref.Genome([n for n, _ in seqs], [s for _, s in seqs], K)
    res = copybacks_ref.copyback_events(g, reads)
    for kind in (H, T):
        assert sum(lf + hf for key, (lf, hf) in res.events.items() if key[0] == kind) >= 200
    assert sum(1 for key in res.events if copybacks_ref.homology(g, *key) > 0) >= 20
    ix = HostIndex.build_mem(K, [("fuzz", [(name, s.encode()) for name, s in seqs])])
    eng = ix.engine()
    try:
        eng.copybacks_enable(2, 12)
        _check(_one(eng, reads), g, res)
        eng.copybacks_enable(0, 12)
        _check(_one(eng, reads), g, copybacks_ref.copyback_events(g, reads, 0), "M=0")
    finally:
        eng.close()
        ix.close()


def test_indels_junctions_and_copybacks_together_give_what_each_gives_alone(world):
    """Pileup, calls, the indel table and span, the junction table and span, the copy-back table and span: an engine with all three
    enabled gives what engines with one of them give."""
    reads, _ = junction_cases.sample_reads(world.g.text)
    reads = reads[:1200] + world.reads[:1200]
    rng = random.Random(5)
    rng.shuffle(reads)
    out = {}
    for name, which in (("all", "ijc"), ("indels", "i"), ("junctions", "j"), ("copybacks", "c")):
        eng = world.ix.engine()
        try:
            if "i" in which:
                eng.indels_enable()
            if "j" in which:
                eng.junctions_enable()
            if "c" in which:
                eng.copybacks_enable()
            eng.sample_begin()
            _packed(eng, 0, reads[:1000])
            _packed(eng, 1, reads[1000:])
            res = eng.sample_finish(2)
            eng.sample_call(2)
            summ, recs = eng.download_calls()
            got = {"pileup": [getattr(res, n).tolist() for n in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk")],
                   "calls": [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.depth, d.af) for d in recs]}
            if "i" in which:
                eng.sample_indels(1, 0)
                isumm, irows = eng.download_indels()
                got["indels"] = ((isumm.records, isumm.anchored, isumm.ref_spanning, isumm.supporting, isumm.discordant), irows, eng.download_indel_span().tolist())
            if "j" in which:
                eng.sample_junctions(1)
                jsumm, jrows = eng.download_junctions()
                got["junctions"] = ((jsumm.records, jsumm.anchored, jsumm.ref_spanning, jsumm.supporting, jsumm.short_, jsumm.backward, jsumm.discordant),
                                    jrows, eng.download_junction_span().tolist())
            if "c" in which:
                eng.sample_copybacks(1)
                csumm, crows = eng.download_copybacks()
                got["copybacks"] = (_tallies(csumm), crows, eng.download_copyback_span().tolist())
            out[name] = got
        finally:
            eng.close()
    for name in ("indels", "junctions", "copybacks"):
        assert out["all"][name] == out[name][name], name
        assert out["all"]["pileup"] == out[name]["pileup"] and out["all"]["calls"] == out[name]["calls"], name
        assert out[name][name][1], name
    want = copybacks_ref.copyback_events(world.g, reads)
    assert out["all"]["copybacks"][1] == copybacks_ref.table_rows(world.g, want)
    assert out["all"]["junctions"][1] == junctions_ref.table_rows(world.g, junctions_ref.junction_events(world.g, reads))
    assert out["all"]["indels"][2] == out["all"]["junctions"][2] == out["all"]["copybacks"][2]   # delta = 0 is one rule


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_copybacks_end_to_end(world, tmp_path, paired):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("cb_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("copybacks", ["--copybacks"]), ("strict", ["--copybacks", "--copyback-max-mismatches", "1", "--copyback-min-reads", "2",
                                                                   "--copyback-min-dist", "360"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("candidate copy-backs" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "cb_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    for name, (M, min_reads, min_dist) in (("copybacks", (2, 5, 0)), ("strict", (1, 2, 360))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".copybacks.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        res = world.res if name == "copybacks" else copybacks_ref.copyback_events(world.g, world.reads, M)
        rows = copybacks_ref.table_rows(world.g, res, min_reads, min_dist)
        assert len(rows) >= 2 and len(rows) < len(res.events)
        assert outs[name][stem + ".copybacks.tsv"].decode() == copybacks_ref.tsv_text(world.g, rows, M, min_reads, min_dist), name
