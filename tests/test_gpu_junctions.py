"""bk_junctions_enable / bk_sample_junctions (bk_junctions.hip) against the Python restatement of the rule (tests/junctions_ref.py):
the whole event table (min_reads 1), the whole span array and every tally must be equal -- the rule is integer arithmetic, no case
is left out.  Then the C ABI's call order, the feature next to the others, and `bronko call --junctions` end to end."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import indel_cases, indels_ref, junction_cases, junctions_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HPV = os.path.join(GOLDEN, "HPV16.fa")
K = 21
TRUSEQ = b"AGATCGGAAGAGC"


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _s(reads):
    return [r.decode() if isinstance(r, bytes) else r for r in reads]


def _finish(eng, n_mates=1, min_reads=1):
    eng.sample_finalize(n_mates)
    eng.sample_junctions(min_reads)
    summ, rows = eng.download_junctions()
    return summ, rows, eng.download_junction_span()


def _tallies(summ):
    return (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.short_, summ.backward, summ.discordant)


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = junctions_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    assert _tallies(summ) == junctions_ref.counters_tuple(res), (what, _tallies(summ), res.counters)
    assert summ.candidates == summ.reported == len(res.events) and summ.overflow == 0, what


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _one(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    return _finish(eng)


class World:
    """HPV16 at k = 21: the index, the genome as the restatement sees it, the 2,000-read sample and what the rule makes of it"""

    def __init__(self):
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.g = junctions_ref.read_fasta(HPV, K)
        self.reads, self.planted = junction_cases.sample_reads(self.g.text)
        self.res = junctions_ref.junction_events(self.g, self.reads)
        assert len(self.res.events) >= 4 and all(v > 0 for v in self.res.counters.values())
        self.eng = self.ix.engine()
        self.eng.junctions_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    seqs = junction_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = junctions_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r, _ in junction_cases.crafted_cases(k)[0]]
    eng = ix.engine()
    try:
        for L, M in ((33, 2), (33, 0), (1, 2), (32, 8), (401, 4), ((1 << 27) - 1, 2)):
            eng.junctions_enable(L, M)
            res = junctions_ref.junction_events(g, reads, L, M)
            assert res.events or L > 1135
            _check(_one(eng, reads, k), g, res, (k, L, M))
    finally:
        eng.close()
        ix.close()


def _junction_reads(w):
    return [r for r in w.reads if junctions_ref.junction_events(w.g, [r]).events]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    reads = (_junction_reads(world)[:n // 2 + 1] + world.reads)[:n]
    res = junctions_ref.junction_events(world.g, reads)
    assert res.events
    _check(_one(world.eng, reads), world.g, res, n)


@pytest.mark.parametrize("order", ["consecutive", "alternating"])
def test_the_queue_carries_over_drains_at_64_and_walks_a_remainder(world, order):
    """200 junction records one after the other: three waves queue 64 and walk them at once, the fourth walks a remainder of 8.
    Alternating with plain records every wave queues 32 and walks them as a remainder.  (Records that wait from one trip of the
    grid to the next need more records than the grid holds: tests/test_gpu_junction_trips.py.)"""
    rng = random.Random(3)
    t = world.g.text
    jn = []
    while len(jn) < 200:
        pos, d = rng.randrange(300, 3000), rng.randrange(33, 3000)
        r = indel_cases.mut_read(t, pos - 70, 150, dele=(pos, d), subs=tuple(rng.sample(range(30, 120), rng.choice((0, 0, 1, 3)))))
        jn.append(r if rng.random() < 0.5 else junctions_ref.revcomp(r))
    if order == "consecutive":
        reads = jn + world.reads[:56]
    else:
        reads = [r for pair in zip(jn, world.reads[200:400]) for r in pair]
    res = junctions_ref.junction_events(world.g, reads)
    assert res.counters["supporting"] + res.counters["discordant"] >= 200 and len(res.events) > 100
    _check(_one(world.eng, reads), world.g, res, order)


def _quals(reads, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in reads:
        qv = rng.integers(30, 41, len(r))
        qv[rng.random(len(r)) < 0.01] = 7
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


@pytest.mark.parametrize("path", ["packed", "packed_ends", "ascii", "ascii_device", "ascii_qual"])
def test_the_sample_through_every_push_path(world, path):
    import torch
    reads = _b(world.reads)
    quals = _quals(reads, 3)
    want = world.res
    if path == "ascii_qual":
        masked = []
        for r, q in zip(reads, quals):
            a = np.frombuffer(r, np.uint8).copy()
            a[np.frombuffer(q, np.uint8) < 33 + 20] = ord("N")
            masked.append(a.tobytes().decode())
        want = junctions_ref.junction_events(world.g, masked)
        assert want.counters["records"] > len(reads) and want.events
    flat = np.frombuffer(b"".join(reads), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_b = torch.from_numpy(np.concatenate([flat, np.zeros(64, np.uint8)])).to("cuda:0")
    keep = []

    def push(eng, a, b):
        if path == "packed":
            _packed(eng, 0, reads[a:b])
        elif path == "packed_ends":
            w, l, e = pack_reads_ends(reads[a:b], K)
            eng.push_reads_ends(0, w, l, e)
        elif path == "ascii":
            eng.push_reads_ascii(0, reads[a:b])
        elif path == "ascii_qual":
            eng.push_reads_ascii(0, reads[a:b], quals[a:b], 20)
        else:
            d_off = torch.from_numpy((off[a:b + 1] - off[a]).copy()).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(d_off)
            eng.push_reads_ascii_device(0, d_b.data_ptr() + int(off[a]), d_off.data_ptr(), b - a, int(off[b] - off[a]), 150)

    for cuts in ([0, len(reads)], [0, 37, 700, 1301, len(reads)]):
        world.eng.sample_begin()
        for a, b in zip(cuts, cuts[1:]):
            push(world.eng, a, b)
        _check(_finish(world.eng), world.g, want, (path, len(cuts) - 1))
        keep.clear()


def test_two_mate_files_add_into_one_table(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads[:900])
    _packed(eng, 1, world.reads[900:])
    _check(_finish(eng, 2), world.g, world.res)


@pytest.mark.parametrize("length", [42, 150, 300])
def test_record_lengths(world, length):
    reads, _ = junction_cases.sample_reads(world.g.text, seed=11, n_reads=600, length=length)
    res = junctions_ref.junction_events(world.g, reads)
    assert res.counters["records"] == 600 and res.counters["anchored"] > 0 and (bool(res.events) == (length >= 150))
    _check(_one(world.eng, reads), world.g, res, length)


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_junctions(1)
        assert ei.value.status == -5
        fork.junctions_enable(33, 2, 12)
        other = junctions_ref.junction_events(world.g, world.reads[:500])
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.junctions_enable(33, 2, 14)
        _check(_one(eng, world.reads[:500]), world.g, junctions_ref.junction_events(world.g, world.reads[:500]))
        eng.junctions_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:500])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_junctions(1)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        eng.junctions_enable(100, 0, 10)
        with pytest.raises(BronkoError) as ei:                     # enabled after the last sample began: that sample has no events
            eng.sample_junctions(1)
        assert ei.value.status == -5
        res = junctions_ref.junction_events(world.g, world.reads[:500], 100, 0)
        assert res.events and res.counters["discordant"] > 0 and res.counters["short"] > 0
        _check(_one(eng, world.reads[:500]), world.g, res)
        # a sample that is begun, pushed and never finalized leaves nothing behind
        eng.sample_begin()
        _packed(eng, 0, world.reads[500:1500])
        _check(_one(eng, world.reads[:500]), world.g, res)
    finally:
        eng.close()


def test_with_primers_and_adapters_set(world):
    from tests.adapter_ref import seen_reads as expected
    rng = np.random.default_rng(5)
    reads = []
    for i, r in enumerate(_b(world.reads[:1200])):               # a third of the reads run into the adapter and a tail
        if i % 3 == 0:
            keep = int(rng.integers(60, 150))
            r = (r[:keep] + TRUSEQ + b"G" * 150)[:150]
        reads.append(r)
    primers = [world.g.text[p:p + 22].encode() for p in range(820, 5600, 397)]
    quals = _quals(reads, 4)
    trimmed, counts, pcounts, _ = expected(reads, quals, [TRUSEQ], 5, 0.1, K, 0, primers, 1)
    assert counts[0] > 200
    res = junctions_ref.junction_events(world.g, _s(trimmed))
    assert res.events and res.counters["ref_spanning"] > 100
    eng = world.ix.engine()
    try:
        eng.adapters_set([TRUSEQ], 5, 0.1)
        eng.primers_set(primers, 1)
        eng.junctions_enable()
        for cuts in ([0, len(reads)], [0, 100, 777, len(reads)]):
            eng.sample_begin()
            for a, b in zip(cuts, cuts[1:]):
                eng.push_reads_ascii(0, reads[a:b])
            _check(_finish(eng), world.g, res, len(cuts))
        w, l, e = pack_reads_ends(reads, K)
        eng.sample_begin()
        eng.push_reads_ends(0, w, l, e)
        _check(_finish(eng), world.g, res, "packed_ends")
    finally:
        eng.close()


def test_a_full_table_is_an_error_not_a_loss(world):
    g = world.g
    reads = [indel_cases.mut_read(g.text, 930 + i, 150, dele=(1000 + i, 40 + i % 7)) for i in range(1500)]   # 1,500 distinct junctions
    res = junctions_ref.junction_events(g, reads)
    assert len(res.events) > 1024
    eng = world.ix.engine()
    try:
        eng.junctions_enable(33, 2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_junctions(1)
        summ = _ffi.JunctionSummary()
        assert eng._L.bk_sample_download_junctions(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate junctions" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_junctions()
        _check(_one(eng, reads[:800]), g, junctions_ref.junction_events(g, reads[:800]))   # the next sample is clean
        eng.junctions_enable(33, 2, 12)
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
        for bad in ((0, 2, 16), (1 << 27, 2, 16), (33, 9, 16), (33, 2, 9), (33, 2, 25)):
            assert status(eng.junctions_enable, *bad) == -1
        assert status(eng.sample_junctions, 1) == -5                  # not enabled
        eng.junctions_enable()
        assert status(eng.sample_junctions, 1) == -5                  # nothing was ever begun
        assert status(eng.download_junctions) == -5 and status(eng.download_junction_span) == -5
        eng.sample_begin()
        assert status(eng.junctions_enable) == -5 and status(eng.junctions_enable, None) == -5   # inside a sample
        assert status(eng.sample_junctions, 1) == -5
        _packed(eng, 0, world.reads[:600])
        eng.sample_finalize(1)
        assert status(eng.download_junctions) == -5                   # finalized, but no report was made
        assert status(eng.sample_junctions, 0) == -1
        res = junctions_ref.junction_events(world.g, world.reads[:600])
        eng.sample_junctions(1)                                       # needs the finalize only, not bk_sample_call
        full = eng.download_junctions()[1]
        assert full == junctions_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_junctions(cap=2)                    # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 6), 0xffffffff, np.uint32), _ffi.JunctionSummary()
        assert eng._L.bk_sample_download_junctions(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert eng._L.bk_sample_download_junctions(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_junctions(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_junction_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1
        seen = set()
        most = max(r[2] + r[3] for r in full)
        for min_reads in (most, most + 1, 2, 1):                      # again with other thresholds on the same sample
            eng.sample_junctions(min_reads)
            summ, rows = eng.download_junctions()
            assert rows == junctions_ref.table_rows(world.g, res, min_reads) and summ.candidates == len(full) and summ.reported == len(rows)
            seen.add(len(rows))
        assert len(seen) >= 3 and 0 in seen and 1 in seen
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_junctions(1)
        assert eng.download_junctions()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_junctions) == -5 and status(eng.sample_junctions, 1) == -5
        eng.sample_finalize(1)
        eng.sample_junctions(1)
        summ, rows = eng.download_junctions()
        assert rows == [] and summ.records == 0 and not eng.download_junction_span().any()
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.junctions_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_every_other_result_is_the_same_with_the_feature_enabled(world):
    """Pileup, calls, the indel table and span, linkage's rows: an engine with junctions enabled gives what one without gives."""
    out = []
    for junctions in (False, True):
        eng = world.ix.engine()
        try:
            eng.indels_enable()
            eng.linkage_enable()
            if junctions:
                eng.junctions_enable()
            eng.sample_begin()
            _packed(eng, 0, world.reads[:1000])
            _packed(eng, 1, world.reads[1000:])
            res = eng.sample_finish(2)
            eng.sample_call(2)
            summ, recs = eng.download_calls()
            eng.sample_indels(1, 0)
            isumm, irows = eng.download_indels()
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        (isumm.records, isumm.anchored, isumm.ref_spanning, isumm.supporting, isumm.discordant, isumm.candidates), irows,
                        eng.download_indel_span().tolist(), sorted(eng.download_link_rows())))
            if junctions:
                eng.sample_junctions(1)
                _check(eng.download_junctions() + (eng.download_junction_span(),), world.g, world.res)
        finally:
            eng.close()
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
        assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
    assert out[0][1:] == out[1][1:] and out[0][1][5] > 0 and out[0][4] and out[0][6]


def test_indels_and_junctions_at_min_len_1_agree_where_they_overlap(world):
    """--indels reports deletions of 1 to 32 bases; --junctions at L = 1 counts the same records as junctions of the same D at the
    same left-normalised cell, with the same reads per strand and the same span at the site."""
    eng = world.ix.engine()
    try:
        eng.indels_enable(32, 2)
        eng.junctions_enable(1, 2)
        t = world.g.text
        reads = list(world.reads)
        for lo, d in ((6000, 32), (6500, 1), (7000, 17)):              # three deletions more, each along and against the reference
            pos = indel_cases._free_pos(t, lo, d)
            r = indel_cases.mut_read(t, pos - 70, 150, dele=(pos, d))
            reads += [r, junctions_ref.revcomp(r), r]
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        eng.sample_junctions(1)
        irows = eng.download_indels()[1]
        jsumm, jrows = eng.download_junctions()
        _check((jsumm, jrows, eng.download_junction_span()), world.g, junctions_ref.junction_events(world.g, reads, 1, 2))
        dels = [(c, ln, f, r, rs) for c, ln, f, r, rs, _ in irows if ln > 0]
        short = [(c, d, f, r, sd) for c, d, f, r, sd, _ in jrows if d <= 32]
        assert dels == short and len(dels) >= 4 and {32, 1} <= {d for _, d, _, _, _ in dels}
        assert np.array_equal(eng.download_indel_span(), eng.download_junction_span())   # delta = 0 is one rule
    finally:
        eng.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_junctions_end_to_end(world, tmp_path, paired):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("jn_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("junctions", ["--junctions"]), ("strict", ["--junctions", "--junction-min-len", "100", "--junction-max-mismatches", "1",
                                                                   "--junction-min-reads", "2"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("candidate junctions" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "jn_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    for name, (L, M, min_reads) in (("junctions", (33, 2, 5)), ("strict", (100, 1, 2))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".junctions.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        res = world.res if name == "junctions" else junctions_ref.junction_events(world.g, world.reads, L, M)
        rows = junctions_ref.table_rows(world.g, res, min_reads)
        assert len(rows) >= 2
        assert outs[name][stem + ".junctions.tsv"].decode() == junctions_ref.tsv_text(world.g, rows, L, M, min_reads), name
