"""bk_indels_enable / bk_sample_indels (bk_indels.hip) against the Python restatement of the rule (tests/indels_ref.py): the whole
event table (min_reads 1, ppm 0), the whole span array and every tally must be equal -- the rule is integer arithmetic, no case is
left out.  Then the C ABI's call order, and `bronko call --indels` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import indel_cases, indels_ref

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


def _finish(eng, n_mates=1, min_reads=1, ppm=0):
    eng.sample_finalize(n_mates)
    eng.sample_indels(min_reads, ppm)
    summ, rows = eng.download_indels()
    return summ, rows, eng.download_indel_span()


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = indels_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    c = res.counters
    assert (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.discordant) == \
        (c["records"], c["anchored"], c["ref_spanning"], c["supporting"], c["discordant"]), what
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
        self.g = indels_ref.read_fasta(HPV, K)
        self.reads, self.planted = indel_cases.sample_reads(self.g.text)
        self.res = indels_ref.indel_events(self.g, self.reads)
        assert len(self.res.events) >= 6 and self.res.counters["ref_spanning"] > 500
        self.eng = self.ix.engine()
        self.eng.indels_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r, _ in indel_cases.crafted_cases(k)]
    eng = ix.engine()
    try:
        for L, M in ((32, 2), (32, 0), (8, 8), (1, 4)):
            eng.indels_enable(L, M)
            res = indels_ref.indel_events(g, reads, L, M)
            assert res.events or L == 1
            _check(_one(eng, reads, k), g, res, (k, L, M))
    finally:
        eng.close()
        ix.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    with_indel = [r for r in world.reads if indels_ref.indel_events(world.g, [r]).events][:n // 2 + 1]
    reads = (with_indel + world.reads)[:n]
    res = indels_ref.indel_events(world.g, reads)
    assert res.events
    _check(_one(world.eng, reads), world.g, res, n)


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
        want = indels_ref.indel_events(world.g, masked)
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


@pytest.mark.parametrize("length", [32, 150, 300])
def test_record_lengths(world, length):
    reads, _ = indel_cases.sample_reads(world.g.text, seed=11, n_reads=400, length=length)
    res = indels_ref.indel_events(world.g, reads)
    assert res.counters["records"] == 400 and (bool(res.events) == (length >= 150)) and (res.counters["anchored"] > 0) == (length >= 2 * K)
    _check(_one(world.eng, reads), world.g, res, length)


def test_k31(world):
    ix = HostIndex.build(31, [HPV])
    eng = ix.engine()
    try:
        g = indels_ref.read_fasta(HPV, 31)
        res = indels_ref.indel_events(g, world.reads[:1000])
        assert res.events
        eng.indels_enable()
        _check(_one(eng, world.reads[:1000], 31), g, res)
    finally:
        eng.close()
        ix.close()


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_indels(1, 0)
        assert ei.value.status == -5
        fork.indels_enable(32, 2, 12)
        other = indels_ref.indel_events(world.g, world.reads[:500])
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.indels_enable(32, 2, 14)
        _check(_one(eng, world.reads[:500]), world.g, indels_ref.indel_events(world.g, world.reads[:500]))
        eng.indels_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:500])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_indels(1, 0)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        eng.indels_enable(4, 0, 10)
        with pytest.raises(BronkoError) as ei:                     # enabled after the last sample began: that sample has no events
            eng.sample_indels(1, 0)
        assert ei.value.status == -5
        res = indels_ref.indel_events(world.g, world.reads[:500], 4, 0)
        assert res.events and res.counters["discordant"] > 0
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
    primers = [world.g.text[p:p + 22].encode() for p in range(520, 1700, 97)]
    quals = _quals(reads, 4)
    trimmed, counts, pcounts, _ = expected(reads, quals, [TRUSEQ], 5, 0.1, K, 0, primers, 1)
    assert counts[0] > 200
    res = indels_ref.indel_events(world.g, _s(trimmed))
    assert res.events and res.counters["ref_spanning"] > 100
    eng = world.ix.engine()
    try:
        eng.adapters_set([TRUSEQ], 5, 0.1)
        eng.primers_set(primers, 1)
        eng.indels_enable()
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
    import random
    rng = random.Random(9)
    g = world.g
    pos = indel_cases._free_pos(g.text, 3000, 1)
    seen, reads = set(), []
    while len(reads) < 1500:                                      # 1,500 distinct inserted sequences at one place
        s = indel_cases._rand(rng, 6)
        if s in seen or s[-1] == g.text[pos - 1]:
            continue
        seen.add(s)
        reads.append(indel_cases.mut_read(g.text, pos - 70, 150, ins=(pos, s)))
    res = indels_ref.indel_events(g, reads)
    assert len(res.events) == 1500
    eng = world.ix.engine()
    try:
        eng.indels_enable(32, 2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        summ = _ffi.IndelSummary()
        assert eng._L.bk_sample_download_indels(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate events" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_indels()
        _check(_one(eng, reads[:800]), g, indels_ref.indel_events(g, reads[:800]))   # the next sample is clean
        eng.indels_enable(32, 2, 12)
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
        for bad in ((0, 2, 16), (33, 2, 16), (32, 9, 16), (32, 2, 9), (32, 2, 25)):
            assert status(eng.indels_enable, *bad) == -1
        assert status(eng.sample_indels, 1, 0) == -5                  # not enabled
        eng.indels_enable()
        assert status(eng.sample_indels, 1, 0) == -5                  # nothing was ever begun
        assert status(eng.download_indels) == -5 and status(eng.download_indel_span) == -5
        eng.sample_begin()
        assert status(eng.indels_enable) == -5 and status(eng.indels_enable, None) == -5   # inside a sample
        assert status(eng.sample_indels, 1, 0) == -5
        _packed(eng, 0, world.reads[:300])
        eng.sample_finalize(1)
        assert status(eng.download_indels) == -5                      # finalized, but no report was made
        assert status(eng.sample_indels, 0, 0) == -1 and status(eng.sample_indels, 1, 1000001) == -1
        res = indels_ref.indel_events(world.g, world.reads[:300])
        eng.sample_indels(1, 0)                                       # needs the finalize only, not bk_sample_call
        full = eng.download_indels()[1]
        assert full == indels_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_indels(cap=2)                       # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 4), 0xff, np.uint64), _ffi.IndelSummary()
        assert eng._L.bk_sample_download_indels(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xff).all()
        assert eng._L.bk_sample_download_indels(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_indels(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_indel_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1
        for min_reads, ppm in ((5, 30000), (1, 1000000), (2, 0)):      # again with other thresholds on the same sample
            eng.sample_indels(min_reads, ppm)
            want = [(c, ln if kd == 0 else -ln, f, r, rs, indels_ref.seq_code(s)) for c, kd, ln, s, f, r, rs in indels_ref.report(world.g, res, min_reads, ppm)]
            summ, rows = eng.download_indels()
            assert rows == want and summ.candidates == len(full)
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_indels(1, 0)
        assert eng.download_indels()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_indels) == -5 and status(eng.sample_indels, 1, 0) == -5
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        summ, rows = eng.download_indels()
        assert rows == [] and summ.records == 0 and not eng.download_indel_span().any()
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.indels_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_every_other_result_is_the_same_with_the_feature_enabled(world):
    plain = world.ix.engine()
    try:
        out = []
        for eng in (plain, world.eng):
            eng.sample_begin()
            _packed(eng, 0, world.reads[:1000])
            _packed(eng, 1, world.reads[1000:])
            res = eng.sample_finish(2)
            eng.sample_call(2)
            summ, recs = eng.download_calls()
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs]))
        for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
            assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
        assert out[0][1:] == out[1][1:] and out[0][1][5] > 0            # (the same summary and records; the sample covers the genome)
    finally:
        plain.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate", ["one", "many"])
@pytest.mark.parametrize("paired", [False, True])
def test_cli_indels_end_to_end(world, tmp_path, paired, inflate):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("ind_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    env = dict(os.environ, BRONKO_INFLATE_THREADS="1") if inflate == "one" else dict(os.environ)
    outs = {}
    for name, extra in (("indels", ["--indels"]), ("strict", ["--indels", "--indel-max-len", "8", "--indel-max-mismatches", "1", "--indel-min-reads", "2",
                                                              "--indel-min-af", "0.1"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra,
                             capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("inflated on" in res.stdout + res.stderr) == (inflate == "many")
        assert ("candidate events" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "ind_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    for name, (L, M, min_reads, ppm) in (("indels", (32, 2, 5, 30000)), ("strict", (8, 1, 2, 100000))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".indels.vcf"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        res = world.res if name == "indels" else indels_ref.indel_events(world.g, world.reads, L, M)
        rows = indels_ref.report(world.g, res, min_reads, ppm)
        assert len(rows) >= 2
        want = indels_ref.vcf_text(world.g, rows, indels_ref.vcf_header(world.g, paths[0], L, M, min_reads, ppm))
        assert outs[name][stem + ".indels.vcf"].decode() == want, name
