"""bk_chimeras_enable / bk_sample_chimeras (bk_chimeras.hip) against the Python restatement of the rule (tests/chimeras_ref.py): the
whole event table (min_reads 1), the whole span array and every tally must be equal -- the rule is integer arithmetic, no case is
left out.  Then the C ABI's call order, the feature next to the others, and `bronko call --chimeras` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import chimera_cases, chimeras_ref
from tests.chimeras_ref import L, R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 21


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _finish(eng, n_mates=1, min_reads=1):
    eng.sample_finalize(n_mates)
    eng.sample_chimeras(min_reads)
    summ, rows = eng.download_chimeras()
    return summ, rows, eng.download_chimera_span()


def _tallies(summ):
    return (summ.records, summ.same_strand, summ.ref_spanning, summ.crossed, summ.supporting, summ.discordant)


def _check(got, g, res, what=""):
    """(summary, rows, span) of the engine against the restatement's result"""
    summ, rows, span = got
    want = chimeras_ref.table_rows(g, res)
    assert rows == want, (what, [r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    sums = np.array(res.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), (what, np.flatnonzero(span != sums)[:5])
    assert _tallies(summ) == chimeras_ref.counters_tuple(res), (what, _tallies(summ), res.counters)
    assert summ.candidates == summ.reported == len(res.events) and summ.overflow == 0, what


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _one(eng, reads, k=K):
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    return _finish(eng)


def _genome(seqs, k):
    return chimeras_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)


def _index(seqs, k, name="fuzz"):
    return HostIndex.build_mem(k, [(name, [(n, s.encode()) for n, s in seqs])])


class World:
    """chimera_cases.fuzz_world at k = 21: the index, the genome as the restatement sees it, 2,000 reads and what the rule makes of them"""

    def __init__(self):
        self.seqs, self.reads = chimera_cases.fuzz_world(n_reads=2000)
        self.ix = _index(self.seqs, K)
        self.g = _genome(self.seqs, K)
        self.res = chimeras_ref.chimera_events(self.g, self.reads)
        assert len(self.res.events) >= 100 and all(v > 0 for v in self.res.counters.values())
        assert {(key[1], key[3]) for key in self.res.events} == {(L, R), (L, L), (R, R), (R, L)}
        self.eng = self.ix.engine()
        self.eng.chimeras_enable()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records_in_one_push(k):
    """Every crafted case of tests/chimera_cases.py (what each is meant to be: tests/test_chimeras_cpu.py), as it is and
    reverse-complemented"""
    seqs = chimera_cases.crafted_genome(k)
    ix = _index(seqs, k, "crafted")
    g = _genome(seqs, k)
    cases = chimera_cases.crafted_cases(k)[0]
    reads = [r for _, r, _ in cases]
    assert min(len(r) for r in reads) == 2 * k - 1 and max(len(r) for r in reads) == 150
    eng = ix.engine()
    try:
        for M in (0, 2, 8):
            eng.chimeras_enable(M)
            res = chimeras_ref.chimera_events(g, reads, M)
            assert len(res.events) >= 20 and (res.counters["discordant"] > 0 or M >= 3)
            _check(_one(eng, reads, k), g, res, (k, M))
        eng.chimeras_enable(2)
        for label, read, _ in cases:                               # ... and one by one, so that a difference names its record
            _check(_one(eng, [read], k), g, chimeras_ref.chimera_events(g, [read], 2), label)
    finally:
        eng.close()
        ix.close()


def _crossed_reads(w):
    return [r for r in w.reads if chimeras_ref.chimera_events(w.g, [r]).counters["crossed"]]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    reads = (_crossed_reads(world)[:n // 2 + 1] + world.reads)[:n]
    res = chimeras_ref.chimera_events(world.g, reads)
    assert res.events
    _check(_one(world.eng, reads), world.g, res, n)


@pytest.mark.parametrize("order", ["consecutive", "alternating"])
def test_the_queue_carries_over_drains_at_64_and_walks_a_remainder(world, order):
    """200 crossed records one after the other: three waves queue 64 and walk them at once, the fourth walks a remainder of 8.
    Alternating with other records every wave queues 32 and walks them as a remainder.  (Records that wait from one trip of the
    grid to the next need more records than the grid holds: tests/test_gpu_chimera_trips.py.)"""
    crossed = _crossed_reads(world)[:200]
    assert len(crossed) == 200
    plain = [r for r in world.reads if chimeras_ref.chimera_events(world.g, [r]).counters["crossed"] == 0]
    reads = crossed + plain[:56] if order == "consecutive" else [r for pair in zip(crossed, plain[:200]) for r in pair]
    res = chimeras_ref.chimera_events(world.g, reads)
    assert res.counters["crossed"] == 200 and len(res.events) > 50
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
    both = set(chimeras_ref.chimera_events(world.g, world.reads[:900]).events) & set(chimeras_ref.chimera_events(world.g, world.reads[900:]).events)
    assert len(both) >= 5                                          # events that both mate files add to


def test_a_read_and_its_reverse_complement_swap_the_counters(world):
    reads = world.reads[:800]
    fwd = _one(world.eng, reads)
    rev = _one(world.eng, [chimeras_ref.revcomp(r) for r in reads])
    assert np.array_equal(fwd[2], rev[2]) and _tallies(fwd[0]) == _tallies(rev[0])
    assert [r[:3] for r in fwd[1]] == [r[:3] for r in rev[1]] and len(fwd[1]) > 50
    assert all((a[3], a[4]) == (b[4], b[3]) for a, b in zip(fwd[1], rev[1]))


def test_500_copies_of_one_read_on_one_event(world):
    read = next(r for r in _crossed_reads(world) if chimeras_ref.chimera_events(world.g, [r]).events)
    res = chimeras_ref.chimera_events(world.g, [read] * 500)
    assert len(res.events) == 1 and sum(next(iter(res.events.values()))) == 500
    _check(_one(world.eng, [read] * 500), world.g, res)


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no table of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_chimeras(1)
        assert ei.value.status == -5
        fork.chimeras_enable(0, 12)
        other = chimeras_ref.chimera_events(world.g, world.reads[:500], 0)
        assert other.events and other.counters["discordant"] > world.res.counters["discordant"] * 500 // 2000
        for e, reads, res in ((world.eng, world.reads, world.res), (fork, world.reads[:500], other), (world.eng, world.reads, world.res)):
            _check(_one(e, reads), world.g, res)
    finally:
        fork.close()


def test_a_full_table_is_an_error_not_a_loss(world):
    g = world.g
    text, first = g.text, g.first
    reads = [chimera_cases.chimera_read(text, first[0] + 300 + i % 1000, L, first[1] + 400 + (i * 7) % 900, R) for i in range(1500)]   # some 1,500 distinct events
    res = chimeras_ref.chimera_events(g, reads)
    assert len(res.events) > 1024
    eng = world.ix.engine()
    try:
        eng.chimeras_enable(2, 10)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        eng.sample_chimeras(1)
        summ = _ffi.ChimeraSummary()
        assert eng._L.bk_sample_download_chimeras(eng.h, C.byref(summ), None, 0) == -1
        assert summ.overflow == 1 and "more than 2^10 distinct candidate chimeras" in eng._L.bk_last_error().decode()
        with pytest.raises(BronkoError):
            eng.download_chimeras()
        _check(_one(eng, reads[:800]), g, chimeras_ref.chimera_events(g, reads[:800]))   # the next sample is clean
        eng.chimeras_enable(2, 12)
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
            assert status(eng.chimeras_enable, *bad) == -1
        assert status(eng.sample_chimeras, 1) == -5                   # not enabled
        eng.chimeras_enable()
        assert status(eng.sample_chimeras, 1) == -5                   # nothing was ever begun
        assert status(eng.download_chimeras) == -5 and status(eng.download_chimera_span) == -5
        eng.sample_begin()
        assert status(eng.chimeras_enable) == -5 and status(eng.chimeras_enable, None) == -5   # inside a sample
        assert status(eng.sample_chimeras, 1) == -5
        _packed(eng, 0, world.reads[:600])
        eng.sample_finalize(1)
        assert status(eng.download_chimeras) == -5                    # finalized, but no report was made
        assert status(eng.sample_chimeras, 0) == -1
        res = chimeras_ref.chimera_events(world.g, world.reads[:600])
        eng.sample_chimeras(1)                                        # needs the finalize only, not bk_sample_call
        full = eng.download_chimeras()[1]
        assert full == chimeras_ref.table_rows(world.g, res) and len(full) > 2
        summ, rows = eng.download_chimeras(cap=2)                     # fewer than there are: `cap` rows, the full count
        assert summ.reported == len(full) and len(rows) == 2 and set(rows) <= set(full)
        raw, s2 = np.full((6, 8), 0xffffffff, np.uint32), _ffi.ChimeraSummary()
        assert eng._L.bk_sample_download_chimeras(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert eng._L.bk_sample_download_chimeras(eng.h, C.byref(s2), None, 100) == 0 and s2.reported == len(full)
        assert eng._L.bk_sample_download_chimeras(eng.h, None, None, 0) == -1
        assert eng._L.bk_sample_download_chimera_span(eng.h, raw.ctypes.data_as(C.c_void_p), 5) == -1   # a cap below bk_total_cells
        seen = set()
        most = max(r[3] + r[4] for r in full)
        for min_reads in (most, most + 1, 5, 2, 1):                   # again with other thresholds on the same sample
            eng.sample_chimeras(min_reads)
            summ, rows = eng.download_chimeras()
            assert rows == chimeras_ref.table_rows(world.g, res, min_reads) and summ.candidates == len(full) and summ.reported == len(rows)
            seen.add(len(rows))
        assert len(seen) >= 3 and 0 in seen
        eng.sample_call(1)                                            # ... and after the call as well
        eng.sample_chimeras(1)
        assert eng.download_chimeras()[1] == full
        eng.sample_begin()                                            # the next sample: the report is no longer this sample's
        assert status(eng.download_chimeras) == -5 and status(eng.sample_chimeras, 1) == -5
        eng.sample_finalize(1)
        eng.sample_chimeras(1)
        summ, rows = eng.download_chimeras()
        assert rows == [] and summ.records == 0 and not eng.download_chimera_span().any()
        # enabled after the sample began: that sample has no events
        eng.chimeras_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:100])
        eng.sample_finalize(1)
        assert status(eng.sample_chimeras, 1) == -5
        eng.chimeras_enable(2, 10)
        assert status(eng.sample_chimeras, 1) == -5
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.chimeras_enable()
        assert ei.value.status == -1 and "one genome file" in str(ei.value)
    finally:
        eng2.close()
        ix2.close()


def test_a_genome_file_of_one_sequence_has_no_events():
    from tests import copybacks_ref
    hpv = os.path.join(GOLDEN, "HPV16.fa")
    ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
    g = copybacks_ref.read_fasta(hpv, K)
    eng = ix.engine()
    try:
        eng.chimeras_enable()
        t = g.text
        reads = [t[s:s + 150] for s in range(100, 4000, 130)] + [t[500:575] + t[3000:3075], chimera_cases.chimera_read(t, 900, L, 2500, L)]
        res = chimeras_ref.chimera_events(g, reads)
        assert not res.events and res.counters["crossed"] == 0 and res.counters["ref_spanning"] == 30 and res.counters["same_strand"] == 31
        _check(_one(eng, reads), g, res)
    finally:
        eng.close()
        ix.close()


def test_every_other_result_is_the_same_with_the_feature_enabled(world):
    """Pileup, calls, the indel, junction, copy-back and duplication tables and spans, linkage's rows: an engine with chimeras enabled
    gives what one without gives."""
    out = []
    for chimeras in (False, True):
        eng = world.ix.engine()
        try:
            eng.indels_enable()
            eng.junctions_enable()
            eng.copybacks_enable()
            eng.duplications_enable()
            eng.linkage_enable()
            if chimeras:
                eng.chimeras_enable()
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
                        (dsumm.records, dsumm.anchored, dsumm.ref_spanning, dsumm.supporting, dsumm.short_, dsumm.forward, dsumm.discordant), drows,
                        eng.download_duplication_span().tolist()))
            if chimeras:
                eng.sample_chimeras(1)
                got = eng.download_chimeras() + (eng.download_chimera_span(),)
                _check(got, world.g, world.res)
                # the siblings ignore the crossed records without a tally: none of theirs counts one as supporting
                assert got[0].supporting > jsumm.supporting + csumm.supporting + dsumm.supporting
        finally:
            eng.close()
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
        assert np.array_equal(getattr(out[0][0], name), getattr(out[1][0], name)), name
    assert out[0][1:] == out[1][1:] and out[0][3][2] > 0 and out[0][10][2] > 0 and out[0][13][2] > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,gz", [(False, False), (False, True), (True, True)])
def test_cli_chimeras_end_to_end(tmp_path, paired, gz):
    """`bronko call --chimeras` on a FASTQ of the crafted records: .chimeras.tsv is the restatement's text, byte for byte, and every
    other output file is what a run without the flag writes"""
    seqs = chimera_cases.crafted_genome(K)
    g = _genome(seqs, K)
    fa = str(tmp_path / "crafted.fa")
    with open(fa, "w") as f:
        for name, s in seqs:
            f.write(">%s\n%s\n" % (name, s))
    db = str(tmp_path / "crafted")
    res = subprocess.run([BRONKO, "build", "-g", fa, "-k", str(K), "-t", "2", "-o", db], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    cases = chimera_cases.crafted_cases(K)[0]
    reads = _b([r for _, r, _ in cases] * 3)                        # every event three times from either cell: six reads
    mates = [reads[:len(reads) // 2], reads[len(reads) // 2:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("ch_R%d.fastq%s" % (m + 1, ".gz" if gz else "")))
        with (gzip.open(p, "wb", compresslevel=1) if gz else open(p, "wb")) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("chimeras", ["--chimeras"]), ("strict", ["--chimeras", "--chimera-max-mismatches", "0", "--chimera-min-reads", "7"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db + ".bkdb"] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("candidate chimeras" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "ch_R1"
    assert stem + ".tsv" in outs["without"] and not any("chimeras" in f for f in outs["without"])
    for name, (M, min_reads) in (("chimeras", (2, 5)), ("strict", (0, 7))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".chimeras.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        r = chimeras_ref.chimera_events(g, [x.decode() for x in reads], M)
        rows = chimeras_ref.table_rows(g, r, min_reads)
        assert (len(rows) >= 10) if name == "chimeras" else (0 < len(rows) < 30)
        assert outs[name][stem + ".chimeras.tsv"].decode() == chimeras_ref.tsv_text(g, rows, M, min_reads, r.counters["supporting"], r.counters["ref_spanning"]), name
