"""bk_breakends_enable / bk_sample_breakends (bk_breakends.hip) against the Python restatement of the rule (tests/breakends_ref.py): the
whole event table (min_reads 1), the whole span array and every tally must be equal -- the rule is integer arithmetic, no case is
left out.  Then the C ABI's call order, the feature next to the others, and `bronko call --breakends` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import breakend_cases, breakends_ref
from tests.breakends_ref import L, R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21
TRUSEQ = b"AGATCGGAAGAGC"


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _s(reads):
    return [r.decode() if isinstance(r, bytes) else r for r in reads]


def _finish(eng, n_mates=1, min_reads=1):
    eng.sample_finalize(n_mates)
    eng.sample_breakends(min_reads)
    summ, rows = eng.download_breakends()
    return summ, rows, eng.download_breakend_span()


def _tallies(summ):
    return (summ.records, summ.one_anchor, summ.ref_spanning, summ.supporting, summ.short_, summ.through, summ.discordant, summ.unplaced)


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = breakends_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    assert _tallies(summ) == breakends_ref.counters_tuple(res), (what, _tallies(summ), res.counters)
    assert summ.candidates == summ.reported == len(res.events) and summ.overflow == 0, what


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _one(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    return _finish(eng)


def _genome(seqs, k):
    return breakends_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)


def _index(seqs, k, name="fuzz"):
    return HostIndex.build_mem(k, [(name, [(n, s.encode()) for n, s in seqs])])


class World:
    """breakend_cases.fuzz_world at k = 21: the index, the genome as the restatement sees it, 2,000 reads and what the rule makes of them"""

    def __init__(self):
        self.seqs, self.reads = breakend_cases.fuzz_world()
        self.ix = _index(self.seqs, K)
        self.g = _genome(self.seqs, K)
        self.res = breakends_ref.breakend_events(self.g, self.reads)
        assert len(self.res.events) >= 100 and all(v > 0 for v in self.res.counters.values())
        assert {key[1] for key in self.res.events} == {L, R}
        self.one = [r for r in self.reads if breakends_ref.breakend_events(self.g, [r]).counters["one_anchor"]]
        self.rest = [r for r in self.reads if not breakends_ref.breakend_events(self.g, [r]).counters["one_anchor"]]
        self.eng = self.ix.engine()
        self.eng.breakends_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    """Every crafted case of tests/breakend_cases.py (what each is meant to be: tests/test_breakends_cpu.py), as it is and
    reverse-complemented, at three settings of (min_clip, max_mismatches)"""
    seqs = breakend_cases.crafted_genome()
    ix = _index(seqs, k, "crafted")
    g = _genome(seqs, k)
    cases = breakend_cases.crafted_cases(k)[0]
    reads = [r for _, r, _ in cases]
    assert min(len(r) for r in reads) == 2 * k - 1 and max(len(r) for r in reads) == 300
    eng = ix.engine()
    try:
        for Cc, M in ((20, 2), (16, 0), (40, 8)):
            eng.breakends_enable(Cc, M)
            res = breakends_ref.breakend_events(g, reads, Cc, M)
            assert len(res.events) >= 10 and (res.counters["short"] > 0 or Cc == 16) and (res.counters["discordant"] > 0 or M == 8)
            _check(_one(eng, reads, k), g, res, (k, Cc, M))
        eng.breakends_enable(20, 2)
        for label, read, _ in cases:                               # ... and one by one, so that a difference names its record
            _check(_one(eng, [read], k), g, breakends_ref.breakend_events(g, [read], 20, 2), label)
    finally:
        eng.close()
        ix.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    reads = (world.one[:n // 2 + 1] + world.reads)[:n]
    res = breakends_ref.breakend_events(world.g, reads)
    assert res.counters["one_anchor"] > 0
    _check(_one(world.eng, reads), world.g, res, n)


@pytest.mark.parametrize("order", ["consecutive", "alternating"])
def test_the_queue_carries_over_drains_at_64_and_walks_a_remainder(world, order):
    """200 one-anchor records one after the other: three waves queue 64 and walk them at once, the fourth walks a remainder of 8.
    Alternating with other records every wave queues 32 and walks them as a remainder.  (Records that wait from one trip of the
    grid to the next need more records than the grid holds: tests/test_gpu_breakend_trips.py.)"""
    one = world.one[:200]
    assert len(one) == 200 and len(world.rest) >= 200
    reads = one + world.rest[:56] if order == "consecutive" else [r for pair in zip(one, world.rest[:200]) for r in pair]
    res = breakends_ref.breakend_events(world.g, reads)
    assert res.counters["one_anchor"] == 200 and len(res.events) > 30
    _check(_one(world.eng, reads), world.g, res, order)


@pytest.mark.parametrize("path", ["packed", "packed_ends", "ascii", "ascii_device"])
def test_the_sample_through_every_push_path(world, path):
    import torch
    reads = _b(world.reads)
    flat = np.frombuffer(b"".join(reads), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_b = torch.from_numpy(np.concatenate([flat, np.zeros(64, np.uint8)])).to("cuda:0")
    keep = []

    def push(eng, a, b):
        if path == "packed":
            _packed(eng, 0, world.reads[a:b])
        elif path == "packed_ends":
            w, l, e = pack_reads_ends(reads[a:b], K)
            eng.push_reads_ends(0, w, l, e)
        elif path == "ascii":
            eng.push_reads_ascii(0, reads[a:b])
        else:
            d_off = torch.from_numpy((off[a:b + 1] - off[a]).copy()).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(d_off)
            eng.push_reads_ascii_device(0, d_b.data_ptr() + int(off[a]), d_off.data_ptr(), b - a, int(off[b] - off[a]), 150)

    for cuts in ([0, len(reads)], [0, 37, 700, 1301, len(reads)]):
        world.eng.sample_begin()
        for a, b in zip(cuts, cuts[1:]):
            push(world.eng, a, b)
        _check(_finish(world.eng), world.g, world.res, (path, len(cuts) - 1))   # (the sample before it left nothing behind)
        keep.clear()


def test_two_mate_files_add_into_one_table(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads[:900])
    _packed(eng, 1, world.reads[900:])
    _check(_finish(eng, 2), world.g, world.res)
    both = set(breakends_ref.breakend_events(world.g, world.reads[:900]).events) & set(breakends_ref.breakend_events(world.g, world.reads[900:]).events)
    assert len(both) >= 5                                          # events that both mate files add to


def test_a_read_and_its_reverse_complement_swap_the_counters(world):
    reads = world.reads[:800]
    fwd = _one(world.eng, reads)
    rev = _one(world.eng, [breakends_ref.revcomp(r) for r in reads])
    assert np.array_equal(fwd[2], rev[2]) and _tallies(fwd[0]) == _tallies(rev[0])
    assert [r[:3] + r[5:] for r in fwd[1]] == [r[:3] + r[5:] for r in rev[1]] and len(fwd[1]) > 50
    assert all((a[3], a[4]) == (b[4], b[3]) for a, b in zip(fwd[1], rev[1]))


def test_500_copies_of_one_read_on_one_event(world):
    read = next(r for r in world.one if breakends_ref.breakend_events(world.g, [r]).events)
    res = breakends_ref.breakend_events(world.g, [read] * 500)
    assert len(res.events) == 1 and sum(next(iter(res.events.values()))) == 500
    _check(_one(world.eng, [read] * 500), world.g, res)


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_breakends(1)
        assert ei.value.status == -5
        fork.breakends_enable(30, 0, 12)
        other = breakends_ref.breakend_events(world.g, world.reads[:500], 30, 0)
        assert other.events and other.counters["discordant"] > world.res.counters["discordant"] * 500 // 2000
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.breakends_enable(20, 2)
        _check(_one(eng, world.reads[:500]), world.g, breakends_ref.breakend_events(world.g, world.reads[:500]))
        eng.breakends_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:100])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_breakends(1)
        assert ei.value.status == -5
        eng.breakends_enable(16, 1, 11)
        res = breakends_ref.breakend_events(world.g, world.reads[:500], 16, 1)
        assert res.counters != breakends_ref.breakend_events(world.g, world.reads[:500]).counters
        _check(_one(eng, world.reads[:500]), world.g, res)
        # a sample that is begun, pushed and never finalized leaves nothing behind
        eng.sample_begin()
        _packed(eng, 0, world.reads[500:1500])
        _check(_one(eng, world.reads[:500]), world.g, res)
    finally:
        eng.close()


def test_a_full_table_is_an_error_not_a_loss(world):
    g = world.g
    import random
    rng, prng = np.random.default_rng(3), random.Random(3)
    cells = rng.choice(np.arange(100, g.cells - 100), 1500, replace=False)                       # some 1,500 distinct events
    reads = [breakend_cases.clipped(g.text, prng, int(c), L, 64, 30) for c in cells]
    res = breakends_ref.breakend_events(g, reads)
    assert len(res.events) > 1024
    eng = world.ix.engine()
    try:
        eng.breakends_enable(20, 2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_breakends(1)
        summ = _ffi.BreakendSummary()
        assert eng._L.bk_sample_download_breakends(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate breakends" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_breakends()
        _check(_one(eng, reads[:800]), g, breakends_ref.breakend_events(g, reads[:800]))   # the next sample is clean
        eng.breakends_enable(20, 2, 12)
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
        for bad in ((15, 2, 16), (65520, 2, 16), (20, 9, 16), (20, 2, 9), (20, 2, 25)):
            assert status(eng.breakends_enable, *bad) == -1
        assert status(eng.sample_breakends, 1) == -5                  # not enabled
        eng.breakends_enable()
        assert status(eng.sample_breakends, 1) == -5                  # nothing was ever begun
        assert status(eng.download_breakends) == -5 and status(eng.download_breakend_span) == -5
        eng.sample_begin()
        assert status(eng.breakends_enable) == -5 and status(eng.breakends_enable, None) == -5   # inside a sample
        assert status(eng.sample_breakends, 1) == -5
        _packed(eng, 0, world.reads[:600])
        eng.sample_finalize(1)
        assert status(eng.download_breakends) == -5                   # finalized, but no report was made
        assert status(eng.sample_breakends, 0) == -1
        res = breakends_ref.breakend_events(world.g, world.reads[:600])
        eng.sample_breakends(1)                                       # needs the finalize only, not bk_sample_call
        full = eng.download_breakends()[1]
        assert full == breakends_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_breakends(cap=2)                    # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 8), 0xffffffff, np.uint32), _ffi.BreakendSummary()
        assert eng._L.bk_sample_download_breakends(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert eng._L.bk_sample_download_breakends(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_breakends(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_breakend_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1   # a cap below bk_total_cells
        assert eng._L.bk_sample_download_breakend_span(eng.h, None, 1 << 20) == -1
        assert eng._L.bk_sample_breakends(eng.h, None) == -1 and eng._L.bk_breakends_enable(None, None) == -1
        seen = set()
        most = max(r[3] + r[4] for r in full)
        for min_reads in (most, most + 1, 5, 2, 1):                   # again with other thresholds on the same sample
            eng.sample_breakends(min_reads)
            summ, rows = eng.download_breakends()
            assert rows == breakends_ref.table_rows(world.g, res, min_reads) and summ.candidates == len(full) and summ.reported == len(rows)
            seen.add(len(rows))
        assert len(seen) >= 3 and 0 in seen
        assert any(r[5] > r[3] + r[4] for r in full)                  # a site's reads over several tags, the ones below the threshold too
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_breakends(1)
        assert eng.download_breakends()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_breakends) == -5 and status(eng.sample_breakends, 1) == -5
        eng.sample_finalize(1)
        eng.sample_breakends(1)
        summ, rows = eng.download_breakends()
        assert rows == [] and summ.records == 0 and not eng.download_breakend_span().any()
        # enabled after the sample began: that sample has no events
        eng.breakends_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:100])
        eng.sample_finalize(1)
        assert status(eng.sample_breakends, 1) == -5
        eng.breakends_enable(20, 2, 10)
        assert status(eng.sample_breakends, 1) == -5
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.breakends_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_an_adapter_clip_vanishes_with_the_adapters_set(world):
    """Plain reads that run into an untrimmed adapter are breakends at as many cells, all with the adapter as their tag; with the
    adapter set the pass reads the trimmed records and they are gone."""
    from tests.adapter_ref import seen_reads as expected
    g = world.g
    t = g.text
    starts = [s for s in range(g.first[1] + 50, g.first[1] + 1000, 19)]
    reads = _b([t[s:s + 100] + TRUSEQ.decode() + "G" * 37 for s in starts] + world.reads[:400])
    quals = [b"I" * len(r) for r in reads]
    trimmed, counts, _, _ = expected(reads, quals, [TRUSEQ], 5, 0.1, K, 0)
    assert counts[0] >= len(starts)
    raw, cut = breakends_ref.breakend_events(g, _s(reads)), breakends_ref.breakend_events(g, _s(trimmed))
    tag = (TRUSEQ.decode() + "GGG")[:16]
    planted = {(s + 99, L, tag) for s in starts}                   # (but for a read that begins in the repeat, or whose next base is the adapter's first)
    assert len(planted & set(raw.events)) >= len(starts) // 2 and not any(key[2] == tag for key in cut.events)
    assert cut.counters["ref_spanning"] >= raw.counters["ref_spanning"] + len(starts) // 2
    eng = world.ix.engine()
    try:
        eng.breakends_enable()
        eng.sample_begin()
        eng.push_reads_ascii(0, reads)
        _check(_finish(eng), g, raw, "untrimmed")
        eng.adapters_set([TRUSEQ], 5, 0.1)
        eng.sample_begin()
        eng.push_reads_ascii(0, reads)
        _check(_finish(eng), g, cut, "ascii")
        w, l, e = pack_reads_ends(reads, K)
        eng.sample_begin()
        eng.push_reads_ends(0, w, l, e)
        _check(_finish(eng), g, cut, "packed_ends")
    finally:
        eng.close()


def test_every_other_result_is_the_same_with_the_feature_enabled(world):
    """Pileup, calls, the indel, junction, copy-back, chimera and duplication tables and spans, linkage's rows: an engine with
    breakends enabled gives what one without gives, and the breakends are those of an engine with nothing else enabled."""
    out = []
    for breakends in (False, True):
        eng = world.ix.engine()
        try:
            eng.indels_enable()
            eng.junctions_enable()
            eng.copybacks_enable()
            eng.chimeras_enable()
            eng.duplications_enable()
            eng.linkage_enable()
            if breakends:
                eng.breakends_enable()
            eng.sample_begin()
            _packed(eng, 0, world.reads[:1000])
            _packed(eng, 1, world.reads[1000:])
            res = eng.sample_finish(2)
            eng.sample_call(2)
            summ, recs = eng.download_calls()
            eng.sample_indels(1, 0)
            isumm, irows = eng.download_indels()
            eng.sample_junctions(1)
            jsumm, jrows = eng.download_junctions()
            eng.sample_copybacks(1)
            csumm, crows = eng.download_copybacks()
            eng.sample_chimeras(1)
            xsumm, xrows = eng.download_chimeras()
            eng.sample_duplications(1)
            dsumm, drows = eng.download_duplications()
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        (isumm.records, isumm.anchored, isumm.ref_spanning, isumm.supporting, isumm.discordant, isumm.candidates), irows,
                        eng.download_indel_span().tolist(), sorted(eng.download_link_rows()),
                        (jsumm.records, jsumm.anchored, jsumm.ref_spanning, jsumm.supporting, jsumm.short_, jsumm.backward, jsumm.discordant), jrows,
                        eng.download_junction_span().tolist(),
                        (csumm.records, csumm.same_strand, csumm.ref_spanning, csumm.switched, csumm.supporting, csumm.discordant), crows,
                        eng.download_copyback_span().tolist(),
                        (xsumm.records, xsumm.same_strand, xsumm.ref_spanning, xsumm.crossed, xsumm.supporting, xsumm.discordant), xrows,
                        eng.download_chimera_span().tolist(),
                        (dsumm.records, dsumm.anchored, dsumm.ref_spanning, dsumm.supporting, dsumm.short_, dsumm.forward, dsumm.discordant), drows,
                        eng.download_duplication_span().tolist()))
            if breakends:
                eng.sample_breakends(1)
                got = eng.download_breakends() + (eng.download_breakend_span(),)
                _check(got, world.g, world.res)
                assert got[0].ref_spanning == jsumm.ref_spanning and np.array_equal(got[2], eng.download_junction_span())   # the same span rule
        finally:
            eng.close()
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
        assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
    assert out[0][1:] == out[1][1:] and out[0][3][2] > 0 and out[0][7][2] > 0
    solo = _one(world.eng, world.reads)                               # this pass alone
    _check(solo, world.g, world.res)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,gz", [(False, False), (True, True)])
def test_cli_breakends_end_to_end(tmp_path, paired, gz):
    """`bronko call --breakends` on a FASTQ of the crafted records: .breakends.tsv is the restatement's text, byte for byte, and every
    other output file is what a run without the flag writes"""
    seqs = breakend_cases.crafted_genome()
    g = _genome(seqs, K)
    fa = str(tmp_path / "crafted.fa")
    with open(fa, "w") as f:
        for name, s in seqs:
            f.write(">%s\n%s\n" % (name, s))
    db = str(tmp_path / "crafted")
    res = subprocess.run([BRONKO, "build", "-g", fa, "-k", str(K), "-t", "2", "-o", db], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    cases = breakend_cases.crafted_cases(K)[0]
    reads = _b([r for _, r, _ in cases] * 3 + [r for _, r, _ in cases[:60]])   # every event three times on either strand, the first ones four times
    mates = [reads[:len(reads) // 2], reads[len(reads) // 2:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("be_R%d.fastq%s" % (m + 1, ".gz" if gz else "")))
        with (gzip.open(p, "wb", compresslevel=1) if gz else open(p, "wb")) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    runs = (("breakends", ["--breakends"]), ("strict", ["--breakends", "--breakend-min-clip", "22", "--breakend-max-mismatches", "0", "--breakend-min-reads", "7"]), ("without", []))
    for name, extra in runs:
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db + ".bkdb"] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("candidate breakends" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "be_R1"
    assert stem + ".tsv" in outs["without"] and not any("breakends" in f for f in outs["without"])
    for name, (Cc, M, min_reads) in (("breakends", (20, 2, 5)), ("strict", (22, 0, 7))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".breakends.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        r = breakends_ref.breakend_events(g, [x.decode() for x in reads], Cc, M)
        rows = breakends_ref.table_rows(g, r, min_reads)
        assert (len(rows) >= 40) if name == "breakends" else (0 < len(rows) < 30)
        assert outs[name][stem + ".breakends.tsv"].decode() == breakends_ref.tsv_text(g, rows, Cc, M, min_reads, breakends_ref.tallies10(r, min_reads)), name
