"""bk_duplications_enable / bk_sample_duplications (bk_duplications.hip) against the Python restatement of the rule
(tests/duplications_ref.py): the whole event table (min_reads 1), the whole span array and every tally must be equal -- the rule is
integer arithmetic, no case is left out.  Then the C ABI's call order, the feature next to the others, and `bronko call
--duplications` end to end."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import duplication_cases, duplications_ref, indels_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HPV = os.path.join(GOLDEN, "HPV16.fa")
K = 21


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _finish(eng, n_mates=1, min_reads=1):
    eng.sample_finalize(n_mates)
    eng.sample_duplications(min_reads)
    summ, rows = eng.download_duplications()
    return summ, rows, eng.download_duplication_span()


def _tallies(summ):
    return (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.short_, summ.forward, summ.discordant)


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = duplications_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    assert _tallies(summ) == duplications_ref.counters_tuple(res), (what, _tallies(summ), res.counters)
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
        self.g = duplications_ref.read_fasta(HPV, K)
        self.reads, self.frequent = duplication_cases.sample_reads(self.g.text)
        self.res = duplications_ref.duplication_events(self.g, self.reads)
        assert len(self.res.events) >= 30 and all(v > 0 for v in self.res.counters.values())
        self.eng = self.ix.engine()
        self.eng.duplications_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    seqs = duplication_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = duplications_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r, _ in duplication_cases.crafted_cases(k)[0]]
    assert min(len(r) for r in reads) == 2 * k - 1 and max(len(r) for r in reads) == 150
    eng = ix.engine()
    try:
        for L, M in ((33, 2), (33, 0), (1, 2), (32, 8), (201, 4), ((1 << 27) - 1, 2)):
            eng.duplications_enable(L, M)
            res = duplications_ref.duplication_events(g, reads, L, M)
            assert res.events or L > 1000
            _check(_one(eng, reads, k), g, res, (k, L, M))
    finally:
        eng.close()
        ix.close()


def test_origin_reads_on_hpv16(world):
    """The last and the first bases of the circular genome: one event (hi, hi - lo) whatever the two lengths are, as long as both hold
    an anchor; with the overhang of a foreign end the record is ignored."""
    g, t = world.g, world.g.text
    n = g.cells
    reads = []
    for left, right in ((32, 32), (32, 118), (118, 32), (75, 75), (21, 43), (43, 21), (21, 129), (129, 21)):
        r = duplication_cases.origin_read(t, left, right)
        reads += [r, duplications_ref.revcomp(r), r]
    res = duplications_ref.duplication_events(g, reads)
    assert list(res.events.items()) == [((n, n), [16, 8])] and res.counters["supporting"] == 24
    rows = duplications_ref.table_rows(g, res)
    assert duplications_ref.tsv_text(g, rows, 33, 2, 1).splitlines()[-1].split("\t") == [g.names[0], "1", str(n), str(n), "16", "8", "24", "0", "0", "1.0000", "0", "1"]
    _check(_one(world.eng, reads), g, res, "origin")
    # one of them among plain reads of the genome's two ends, which span cells next to the origin but never the origin itself
    plain = [t[:150], t[n - 150:], t[10:160], duplications_ref.revcomp(t[n - 170:n - 20])]
    res = duplications_ref.duplication_events(g, reads[:1] + plain)
    assert res.counters["ref_spanning"] == 4 and duplications_ref.table_rows(g, res) == [(n, n, 1, 0, 0, 0)]
    _check(_one(world.eng, reads[:1] + plain), g, res, "origin and plain")
    # eight foreign bases at either end: dL < lo, dR + n > hi
    x8 = "ACCAGTCA"
    over = [x8 + t[:60] + t[10:92], t[n - 92:n - 10] + t[n - 60:] + x8]
    over += [duplications_ref.revcomp(r) for r in over]
    res = duplications_ref.duplication_events(g, over)
    assert not res.events and res.counters["anchored"] == 4 and duplications_ref.counters_tuple(res)[2:] == (0, 0, 0, 0, 0)
    _check(_one(world.eng, over), g, res, "overhang")


def _event_reads(w):
    return [r for r in w.reads if duplications_ref.duplication_events(w.g, [r]).events]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    reads = (_event_reads(world)[:n // 2 + 1] + world.reads)[:n]
    res = duplications_ref.duplication_events(world.g, reads)
    assert res.events
    _check(_one(world.eng, reads), world.g, res, n)


@pytest.mark.parametrize("order", ["consecutive", "alternating"])
def test_the_queue_carries_over_drains_at_64_and_walks_a_remainder(world, order):
    """200 backward-jump records one after the other: three waves queue 64 and walk them at once, the fourth walks a remainder of 8.
    Alternating with plain records every wave queues 32 and walks them as a remainder.  (Records that wait from one trip of the
    grid to the next need more records than the grid holds: tests/test_gpu_duplication_trips.py.)"""
    rng = random.Random(3)
    t = world.g.text
    dup = []
    while len(dup) < 200:
        e = rng.randrange(33, 3000)
        pos = rng.randrange(e + 100, 7700)
        r = duplication_cases.dup_read(t, pos, e, subs=tuple(rng.sample(range(30, 120), rng.choice((0, 0, 1, 3)))))
        dup.append(r if rng.random() < 0.5 else duplications_ref.revcomp(r))
    plain = [r for r in world.reads if duplications_ref.duplication_events(world.g, [r]).counters["ref_spanning"]]
    if order == "consecutive":
        reads = dup + plain[:56]
    else:
        reads = [r for pair in zip(dup, plain[:200]) for r in pair]
    res = duplications_ref.duplication_events(world.g, reads)
    assert res.counters["supporting"] + res.counters["discordant"] >= 200 and len(res.events) > 100
    _check(_one(world.eng, reads), world.g, res, order)


@pytest.mark.parametrize("path", ["packed_ends", "ascii", "ascii_device"])
def test_the_sample_through_every_push_path(world, path):
    import torch
    reads = _b(world.reads)
    flat = np.frombuffer(b"".join(reads), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_b = torch.from_numpy(np.concatenate([flat, np.zeros(64, np.uint8)])).to("cuda:0")
    keep = []

    def push(eng, a, b):
        if path == "packed_ends":
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
        _check(_finish(world.eng), world.g, world.res, (path, len(cuts) - 1))
        keep.clear()


def test_two_mate_files_add_into_one_table(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads[:900])
    _packed(eng, 1, world.reads[900:])
    _check(_finish(eng, 2), world.g, world.res)
    both = {key for key in duplications_ref.duplication_events(world.g, world.reads[:900]).events} & \
           {key for key in duplications_ref.duplication_events(world.g, world.reads[900:]).events}
    assert len(both) >= 5                                          # events that both mate files add to


@pytest.mark.parametrize("length", [64, 100, 150])
def test_record_lengths(world, length):
    reads, _ = duplication_cases.sample_reads(world.g.text, seed=11, n_reads=600, length=length)
    res = duplications_ref.duplication_events(world.g, reads)
    assert res.counters["records"] == 600 and res.counters["anchored"] > 0 and res.events
    _check(_one(world.eng, reads), world.g, res, length)


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_duplications(1)
        assert ei.value.status == -5
        fork.duplications_enable(33, 2, 12)
        other = duplications_ref.duplication_events(world.g, world.reads[:500])
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.duplications_enable(33, 2, 14)
        _check(_one(eng, world.reads[:500]), world.g, duplications_ref.duplication_events(world.g, world.reads[:500]))
        eng.duplications_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:500])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_duplications(1)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        eng.duplications_enable(100, 0, 10)
        with pytest.raises(BronkoError) as ei:                     # enabled after the last sample began: that sample has no events
            eng.sample_duplications(1)
        assert ei.value.status == -5
        res = duplications_ref.duplication_events(world.g, world.reads[:500], 100, 0)
        assert res.events and res.counters["discordant"] > 0 and res.counters["short"] > 0
        _check(_one(eng, world.reads[:500]), world.g, res)
        # a sample that is begun, pushed and never finalized leaves nothing behind
        eng.sample_begin()
        _packed(eng, 0, world.reads[500:1500])
        _check(_one(eng, world.reads[:500]), world.g, res)
    finally:
        eng.close()


def test_a_full_table_is_an_error_not_a_loss(world):
    g = world.g
    reads = [duplication_cases.dup_read(g.text, 1000 + i, 40 + i % 7) for i in range(1500)]   # some 1,500 distinct events
    res = duplications_ref.duplication_events(g, reads)
    assert len(res.events) > 1024
    eng = world.ix.engine()
    try:
        eng.duplications_enable(33, 2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_duplications(1)
        summ = _ffi.DuplicationSummary()
        assert eng._L.bk_sample_download_duplications(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate duplications" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_duplications()
        _check(_one(eng, reads[:800]), g, duplications_ref.duplication_events(g, reads[:800]))   # the next sample is clean
        eng.duplications_enable(33, 2, 12)
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
            assert status(eng.duplications_enable, *bad) == -1
        assert status(eng.sample_duplications, 1) == -5               # not enabled
        eng.duplications_enable()
        assert status(eng.sample_duplications, 1) == -5               # nothing was ever begun
        assert status(eng.download_duplications) == -5 and status(eng.download_duplication_span) == -5
        eng.sample_begin()
        assert status(eng.duplications_enable) == -5 and status(eng.duplications_enable, None) == -5   # inside a sample
        assert status(eng.sample_duplications, 1) == -5
        _packed(eng, 0, world.reads[:600])
        eng.sample_finalize(1)
        assert status(eng.download_duplications) == -5                # finalized, but no report was made
        assert status(eng.sample_duplications, 0) == -1
        res = duplications_ref.duplication_events(world.g, world.reads[:600])
        eng.sample_duplications(1)                                    # needs the finalize only, not bk_sample_call
        full = eng.download_duplications()[1]
        assert full == duplications_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_duplications(cap=2)                 # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 6), 0xffffffff, np.uint32), _ffi.DuplicationSummary()
        assert eng._L.bk_sample_download_duplications(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert eng._L.bk_sample_download_duplications(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_duplications(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_duplication_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1
        seen = set()
        most = max(r[2] + r[3] for r in full)
        for min_reads in (most, most + 1, 5, 2, 1):                   # again with other thresholds on the same sample
            eng.sample_duplications(min_reads)
            summ, rows = eng.download_duplications()
            assert rows == duplications_ref.table_rows(world.g, res, min_reads) and summ.candidates == len(full) and summ.reported == len(rows)
            seen.add(len(rows))
        assert len(seen) >= 4 and 0 in seen and 1 in seen
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_duplications(1)
        assert eng.download_duplications()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_duplications) == -5 and status(eng.sample_duplications, 1) == -5
        eng.sample_finalize(1)
        eng.sample_duplications(1)
        summ, rows = eng.download_duplications()
        assert rows == [] and summ.records == 0 and not eng.download_duplication_span().any()
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.duplications_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_every_other_result_is_the_same_with_the_feature_enabled(world):
    """Pileup, calls, the indel, junction and copy-back tables and spans, linkage's rows: an engine with duplications enabled gives
    what one without gives -- and the junction pass's `backward` tally follows its own cell rule."""
    out = []
    for duplications in (False, True):
        eng = world.ix.engine()
        try:
            eng.indels_enable()
            eng.junctions_enable()
            eng.copybacks_enable()
            eng.linkage_enable()
            if duplications:
                eng.duplications_enable()
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
            out.append((res, (summ.file_id, summ.n_records, summ.n_major, summ.n_minor, summ.covered, summ.coverage),
                        [(d.seq_id, d.pos, d.ref_base, d.alt_base, d.fwd_ref, d.rev_ref, d.fwd_alt, d.rev_alt, d.depth, d.af, d.sor) for d in recs],
                        (isumm.records, isumm.anchored, isumm.ref_spanning, isumm.supporting, isumm.discordant, isumm.candidates), irows,
                        eng.download_indel_span().tolist(), sorted(eng.download_link_rows()),
                        (jsumm.records, jsumm.anchored, jsumm.ref_spanning, jsumm.supporting, jsumm.short_, jsumm.backward, jsumm.discordant), jrows,
                        eng.download_junction_span().tolist(), (csumm.records, csumm.same_strand, csumm.ref_spanning, csumm.switched), crows))
            if duplications:
                eng.sample_duplications(1)
                got = eng.download_duplications() + (eng.download_duplication_span(),)
                _check(got, world.g, world.res)
                # the origin reads overhang the junction rule's cells: they are in no tally of it
                assert 0 < jsumm.backward < got[0].supporting + got[0].discordant
        finally:
            eng.close()
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
        assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
    assert out[0][1:] == out[1][1:] and out[0][1][5] > 0 and out[0][6] and out[0][8]


def test_indels_and_duplications_at_min_len_1_agree_where_they_overlap(world):
    """--indels reports insertions of 1 to 32 bases; a tandem duplication of that length that lies whole inside the read is one, and
    --duplications at L = 1 counts the same records as events of the same length whose first duplicated cell is the insertion's
    cell, with the same reads per strand, the inserted bases the duplicated ones."""
    eng = world.ix.engine()
    try:
        eng.indels_enable(32, 0)
        eng.duplications_enable(1, 0)
        t = world.g.text
        reads, planted = [], []
        for lo, e in ((1500, 32), (2500, 1), (3500, 17), (4500, 6)):   # each along and against the reference
            pos = duplication_cases.free_pos(t, lo, e)
            r = duplication_cases.dup_read(t, pos, e)
            reads += [r, duplications_ref.revcomp(r), r]
            planted.append((pos, e))
        reads += [t[s:s + 150] for s in range(1400, 4600, 100)]
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_indels(1, 0)
        eng.sample_duplications(1)
        irows = eng.download_indels()[1]
        dsumm, drows = eng.download_duplications()
        _check((dsumm, drows, eng.download_duplication_span()), world.g, duplications_ref.duplication_events(world.g, reads, 1, 0))
        ins = sorted((c, -ln, f, r, seq) for c, ln, f, r, _, seq in irows if ln < 0)
        dup = sorted((c - e, e, f, r, indels_ref.seq_code(t[c - e:c])) for c, e, f, r, _, _ in drows)
        assert ins == dup and [x[:4] for x in dup] == sorted((pos - e, e, 2, 1) for pos, e in planted)
        assert np.array_equal(eng.download_indel_span(), eng.download_duplication_span())   # delta = 0 is one rule inside a sequence
    finally:
        eng.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_duplications_end_to_end(world, tmp_path, paired):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("dp_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("duplications", ["--duplications"]), ("strict", ["--duplications", "--duplication-min-len", "100", "--duplication-max-mismatches", "1",
                                                                         "--duplication-min-reads", "2"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("candidate duplications" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "dp_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    for name, (L, M, min_reads) in (("duplications", (33, 2, 5)), ("strict", (100, 1, 2))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".duplications.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        res = world.res if name == "duplications" else duplications_ref.duplication_events(world.g, world.reads, L, M)
        rows = duplications_ref.table_rows(world.g, res, min_reads)
        assert len(rows) >= 4 and (world.g.cells, world.g.cells) in {r[:2] for r in rows}
        assert outs[name][stem + ".duplications.tsv"].decode() == duplications_ref.tsv_text(world.g, rows, L, M, min_reads), name
