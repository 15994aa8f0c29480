"""bk_link_enable / bk_sample_linkage (bk_linkage.hip) against the Python restatement of the rule (tests/linkage_ref.py): the row
store as a multiset, every counter of every pair and the four tallies must be equal -- the rule is integer arithmetic, no case is
left out.  Then the row store's growth, the C ABI's call order, and `bronko call --linkage` end to end."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import indel_cases, indels_ref, linkage_cases, linkage_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HPV = os.path.join(GOLDEN, "HPV16.fa")
K = 21
TRUSEQ = b"AGATCGGAAGAGC"
LDS_PAIRS = 512                      # kLinkLdsPairs: a counter table of more pairs takes the global path


def _b(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def _s(reads):
    return [r.decode() if isinstance(r, bytes) else r for r in reads]


def _packed(eng, mate, reads, k=K):
    w, l = pack_reads(_b(reads), k)
    eng.push_reads(mate, w, l)


def _check(eng, g, rows, tallies, sites, max_dist=1000, what=""):
    """The finalized sample's row store, tallies and counters against the restatement's"""
    got = eng.download_link_rows()
    assert got == rows, (what, len(got), len(rows), [r for r in got if r not in rows][:3], [r for r in rows if r not in got][:3])
    eng.sample_linkage(sites, max_dist)
    summ, pairs = eng.download_linkage()
    assert (summ.records, summ.placed, summ.unplaced, summ.discordant) == \
        (tallies["records"], tallies["placed"], tallies["unplaced"], tallies["discordant"]), what
    want = linkage_ref.link_count(g, rows, sites, max_dist)
    assert (summ.n_sites, summ.max_dist, summ.n_pairs) == (len(sites), max_dist, len(want)), what
    assert pairs == want, (what, [(p, w) for p, w in zip(pairs, want) if p != w][:3])
    return pairs


def _one(eng, g, reads, M, sites, k=K, max_dist=1000, what=""):
    rows, t = linkage_ref.link_rows(g, reads, M)
    eng.sample_begin()
    _packed(eng, 0, reads, k)
    eng.sample_finalize(1)
    return _check(eng, g, rows, t, sites, max_dist, what)


class World(linkage_cases.Planted):
    """... with the index and an engine that has linkage enabled"""

    def __init__(self):
        super().__init__(K)
        self.ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
        self.eng = self.ix.engine()
        self.eng.linkage_enable()
        self.every = list(range(linkage_cases.SAMPLE_P - 100, linkage_cases.SAMPLE_P + 300))   # 400 cells: many sites in a row
        self.every_pairs = linkage_ref.link_count(self.g, self.rows, self.every, 1000)
        assert len(self.every_pairs) > LDS_PAIRS >= len(self.pairs) > 0


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()
    w.ix.close()


@pytest.mark.parametrize("k", [21, 31])
def test_crafted_records(k):
    seqs = indel_cases.crafted_genome(k)
    ix = HostIndex.build_mem(k, [("crafted", [(name, s.encode()) for name, s in seqs])])
    g = indels_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], k)
    reads = [r for _, r in linkage_cases.crafted_cases(k)]
    sites = linkage_cases.crafted_sites(k)
    eng = ix.engine()
    try:
        for M in (0, 2, 8):
            eng.linkage_enable(M, 16)
            pairs = _one(eng, g, reads, M, sites, k, what=(k, M))
            assert sum(sum(c) for _, _, c in pairs) > 50
        _one(eng, g, reads, 8, sites, k, max_dist=2, what=(k, "dist 2"))
    finally:
        eng.close()
        ix.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_record_a_full_wave_and_one_more(world, n):
    placed = [r for r in world.reads if linkage_ref.place(world.g, linkage_ref.records_of(r, K)[0], 8)[0] == "placed"]
    _one(world.eng, world.g, placed[:n], 8, world.sites, what=n)


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
    rows, t = world.rows, world.tallies
    if path == "ascii_qual":
        masked = []
        for r, q in zip(reads, quals):
            a = np.frombuffer(r, np.uint8).copy()
            a[np.frombuffer(q, np.uint8) < 33 + 20] = ord("N")
            masked.append(a.tobytes().decode())
        rows, t = linkage_ref.link_rows(world.g, masked, 8)
        assert t["records"] > len(reads) and t["placed"] > 500
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
        world.eng.sample_finalize(1)
        _check(world.eng, world.g, rows, t, world.sites, what=(path, len(cuts) - 1))
        keep.clear()


def test_two_mate_files_add_into_one_store(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads[:900])
    _packed(eng, 1, world.reads[900:])
    eng.sample_finalize(2)
    _check(eng, world.g, world.rows, world.tallies, world.sites)


@pytest.mark.parametrize("length", [32, 150, 300])
def test_record_lengths(world, length):
    reads, _, _ = linkage_cases.sample_reads(world.g.text, seed=11, n_reads=400, length=length)
    rows, t = linkage_ref.link_rows(world.g, reads, 8)
    assert t["records"] == 400 and (t["placed"] > 100) == (length >= 2 * K)
    _one(world.eng, world.g, reads, 8, world.sites, what=length)


def test_lds_path_global_path_and_both_agree(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads)
    eng.sample_finalize(1)
    three = world.hap1[:3]
    small = _check(eng, world.g, world.rows, world.tallies, three, what="3 sites")       # 3 pairs: the table is privatised in LDS
    assert len(small) == 3 and all(sum(c) > 50 for _, _, c in small)   # (2,000 reads of 150 over 1,950 starts: about 87 cover two cells 63 apart)
    eng.sample_linkage(world.every, 1000)                                                  # 400 sites: global atomics
    summ, large = eng.download_linkage()
    assert summ.n_pairs == len(world.every_pairs) > LDS_PAIRS and large == world.every_pairs
    by = {(a, b): c for a, b, c in large}
    assert all(by[(a, b)] == c for a, b, c in small)                                       # the shared pairs under both paths
    assert max(sum(1 for s in world.every if r[0] <= s < r[0] + r[1]) for r in world.rows) == 150   # a row that covers 150 sites


def test_sample_linkage_again_with_another_distance(world):
    eng = world.eng
    eng.sample_begin()
    _packed(eng, 0, world.reads)
    eng.sample_finalize(1)
    for dist in (1000, 3, 65519, 60, 1000):                                                # the counters are zeroed each time
        _check(eng, world.g, world.rows, world.tallies, world.sites, dist, what=dist)
    eng.sample_linkage([], 10)
    summ, pairs = eng.download_linkage()
    assert pairs == [] and summ.n_pairs == 0 and summ.placed == world.tallies["placed"]
    summ, pairs = eng.download_linkage(cap=2)
    assert pairs == []
    eng.sample_linkage(world.sites, 1000)
    summ, pairs = eng.download_linkage(cap=2)                                              # fewer than there are: `cap` rows, the full count
    assert summ.n_pairs == len(world.pairs) and pairs == world.pairs[:2]
    assert eng.download_link_rows(cap=5) == sorted(eng.download_link_rows(cap=5)) and len(eng.download_link_rows(cap=5)) == 5


def test_the_row_store_grows_and_loses_nothing(world):
    eng = world.ix.engine()
    try:
        eng.linkage_enable(8, 64)                                                          # 64 rows, 2,000 records, four pushes
        for _ in range(2):                                                                 # (the second sample starts from the grown store)
            eng.sample_begin()
            for a, b in ((0, 37), (37, 700), (700, 1301), (1301, 2000)):
                _packed(eng, 0, world.reads[a:b])
            eng.sample_finalize(1)
            _check(eng, world.g, world.rows, world.tallies, world.sites)
        eng.linkage_enable(2, 1)
        rows, t = linkage_ref.link_rows(world.g, world.reads, 2)
        assert t["discordant"] > 100
        eng.sample_begin()
        for a in range(0, 2000, 250):
            _packed(eng, a // 1000, world.reads[a:a + 250])
        eng.sample_finalize(2)
        _check(eng, world.g, rows, t, world.sites)
    finally:
        eng.close()


def test_an_engine_its_fork_and_the_engine_again(world):
    fork = world.eng.fork()
    try:
        fork.sample_begin()                                        # a fork has no row store of its parent's
        _packed(fork, 0, world.reads[:100])
        fork.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            fork.sample_linkage(world.sites)
        assert ei.value.status == -5
        fork.linkage_enable(8, 128)
        for e, reads in ((world.eng, world.reads), (fork, world.reads[:500]), (world.eng, world.reads)):
            _one(e, world.g, reads, 8, world.sites)
    finally:
        fork.close()


def test_enable_disable_enable_and_an_abandoned_sample(world):
    eng = world.ix.engine()
    try:
        eng.linkage_enable(8, 256)
        _one(eng, world.g, world.reads[:500], 8, world.sites)
        eng.linkage_enable(None)
        eng.sample_begin()
        _packed(eng, 0, world.reads[:500])
        eng.sample_finalize(1)
        with pytest.raises(BronkoError) as ei:
            eng.sample_linkage(world.sites)
        assert ei.value.status == -5 and "enabled" in str(ei.value)
        eng.linkage_enable(0, 256)
        with pytest.raises(BronkoError) as ei:                     # enabled after the last sample began: that sample has no rows
            eng.sample_linkage(world.sites)
        assert ei.value.status == -5
        _one(eng, world.g, world.reads[:500], 0, world.sites)
        eng.sample_begin()                                         # begun, pushed and never finalized: nothing is left behind
        _packed(eng, 0, world.reads[500:1500])
        _one(eng, world.g, world.reads[:500], 0, world.sites)
    finally:
        eng.close()


@pytest.mark.parametrize("order", ["indels_first", "linkage_first", "indels_dropped"])
def test_with_indels_enabled_as_well(world, order):
    reads, _ = indel_cases.sample_reads(world.g.text)
    reads = reads[:1000] + world.reads[:1000]
    res = indels_ref.indel_events(world.g, reads)
    assert len(res.events) >= 6
    rows, t = linkage_ref.link_rows(world.g, reads, 8)
    eng = world.ix.engine()
    try:
        if order == "linkage_first":
            eng.linkage_enable(8, 512)
            eng.indels_enable()
        else:
            eng.indels_enable()
            eng.linkage_enable(8, 512)
        if order == "indels_dropped":                              # the anchor tables stay while either feature holds them
            eng.indels_enable(None)
        eng.sample_begin()
        _packed(eng, 0, reads)
        eng.sample_finalize(1)
        if order != "indels_dropped":
            eng.sample_indels(1, 0)
            summ, irows = eng.download_indels()
            assert irows == indels_ref.table_rows(world.g, res)
            span = eng.download_indel_span()
            assert np.array_equal(span, np.array(res.span_sums()[:world.g.cells], np.int64).astype(np.uint32))
            c = res.counters
            assert (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.discordant) == \
                (c["records"], c["anchored"], c["ref_spanning"], c["supporting"], c["discordant"])
        _check(eng, world.g, rows, t, world.sites, what=order)
        if order == "linkage_first":                               # ... and indels alone once linkage is dropped
            eng.linkage_enable(None)
            eng.sample_begin()
            _packed(eng, 0, reads)
            eng.sample_finalize(1)
            eng.sample_indels(1, 0)
            assert eng.download_indels()[1] == indels_ref.table_rows(world.g, res)
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
    primers = [world.g.text[p:p + 22].encode() for p in range(1720, 3700, 97)]
    quals = _quals(reads, 4)
    trimmed, counts, pcounts, _ = expected(reads, quals, [TRUSEQ], 5, 0.1, K, 0, primers, 1)
    assert counts[0] > 200
    rows, t = linkage_ref.link_rows(world.g, _s(trimmed), 8)
    assert t["placed"] > 500
    eng = world.ix.engine()
    try:
        eng.adapters_set([TRUSEQ], 5, 0.1)
        eng.primers_set(primers, 1)
        eng.linkage_enable(8, 100)
        for cuts in ([0, len(reads)], [0, 100, 777, len(reads)]):
            eng.sample_begin()
            for a, b in zip(cuts, cuts[1:]):
                eng.push_reads_ascii(0, reads[a:b])
            eng.sample_finalize(1)
            _check(eng, world.g, rows, t, world.sites, what=len(cuts))
        w, l, e = pack_reads_ends(reads, K)
        eng.sample_begin()
        eng.push_reads_ends(0, w, l, e)
        eng.sample_finalize(1)
        _check(eng, world.g, rows, t, world.sites, what="packed_ends")
    finally:
        eng.close()


def test_call_order_and_parameters(world):
    eng = world.ix.engine()

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        for bad in ((9, 64), (8, 0)):
            assert status(eng.linkage_enable, *bad)[0] == -1
        assert status(eng.sample_linkage, world.sites)[0] == -5      # not enabled
        eng.linkage_enable()
        assert status(eng.sample_linkage, world.sites)[0] == -5      # nothing was ever begun
        assert status(eng.download_linkage)[0] == -5 and status(eng.download_link_rows)[0] == -5
        eng.sample_begin()
        assert status(eng.linkage_enable)[0] == -5 and status(eng.linkage_enable, None)[0] == -5   # inside a sample
        assert status(eng.sample_linkage, world.sites)[0] == -5
        _packed(eng, 0, world.reads[:300])
        assert status(eng.sample_linkage, world.sites)[0] == -5      # before the finalize
        assert status(eng.download_link_rows)[0] == -5
        eng.sample_finalize(1)
        rows, t = linkage_ref.link_rows(world.g, world.reads[:300], 8)
        cells = world.g.cells
        for bad, word in (([5, 5], "ascending"), ([7, 5], "ascending"), ([1, 2, cells], "cell"), (list(range(65537)), "65536")):
            st, msg = status(eng.sample_linkage, bad, 1000)
            assert st == -1 and word in msg, (bad[:3], msg)
        for dist in (0, 65520):
            assert status(eng.sample_linkage, world.sites, dist)[0] == -1
        many = list(range(0, 7000))                                   # 7,000 sites within 1,000 cells of each other: 6.5 M pairs
        st, msg = status(eng.sample_linkage, many, 1000)
        n_pairs = sum(min(1000, 6999 - i) for i in range(7000))
        assert st == -1 and str(n_pairs) in msg and n_pairs > 1 << 20
        summ, pairs = eng.download_linkage()                          # no launch was made, nothing was counted
        assert pairs == [] and summ.n_pairs == 0 and summ.placed == t["placed"]
        _check(eng, world.g, rows, t, world.sites)                    # needs the finalize only, not bk_sample_call
        eng.sample_call(1)
        _check(eng, world.g, rows, t, world.sites, 50)                # ... and after the call as well
        raw, s2 = np.full((6, 18), 0xffffffff, np.uint32), _ffi.LinkSummary()
        assert eng._L.bk_sample_download_linkage(eng.h, C.byref(s2), raw.ctypes.data_as(C.c_void_p), 2) == 0 and (raw[2:] == 0xffffffff).all()
        assert eng._L.bk_sample_download_linkage(eng.h, None, None, 0) == -1
        eng.sample_begin()                                            # the next sample: nothing is this sample's yet
        assert status(eng.download_linkage)[0] == -5 and status(eng.sample_linkage, world.sites)[0] == -5
        eng.sample_finalize(1)
        eng.sample_linkage(world.sites)
        summ, pairs = eng.download_linkage()
        assert summ.records == 0 and summ.placed == 0 and len(pairs) == len(world.pairs) and not any(any(c) for _, _, c in pairs)
        assert eng.download_link_rows() == []
    finally:
        eng.close()
    sars = [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")]
    ix2 = HostIndex.build(K, sars)
    eng2 = ix2.engine()
    try:
        with pytest.raises(BronkoError) as ei:
            eng2.linkage_enable()
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
        assert out[0][1:] == out[1][1:] and out[0][1][1] > 0            # (the same summary and records; the sample has calls)
    finally:
        plain.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_cli_linkage_end_to_end(world, tmp_path, paired):
    reads = _b(world.reads)
    mates = [reads[:1000], reads[1000:]] if paired else [reads]
    paths = []
    for m, rd in enumerate(mates):
        p = str(tmp_path / ("lnk_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(rd):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(GOLDEN, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    outs = {}
    for name, extra in (("linkage", ["--linkage"]), ("strict", ["--linkage", "--link-max-mismatches", "3", "--link-max-dist", "200", "--link-min-reads", "2"]),
                        ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra,
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("pairs counted" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "lnk_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv"}
    recs = linkage_ref.parse_vcf(world.g, outs["without"][stem + ".vcf"].decode())
    sites = linkage_ref.sites_of(recs)
    assert len(sites) >= 2                                           # (the sites are whatever the run's own VCF holds)
    seen = set()
    for name, (M, D, N) in (("linkage", (8, 1000, 1)), ("strict", (3, 200, 2))):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".linkage.tsv"}
        for f in outs["without"]:                                  # every other output does not know of the flag
            assert outs[name][f] == outs["without"][f], (name, f)
        rows, _ = linkage_ref.link_rows(world.g, world.reads, M)
        want = linkage_ref.tsv_text(world.g, recs, linkage_ref.link_count(world.g, rows, sites, D), M, D, N)
        assert want.count("\n") >= 5                                # at least one pair of the VCF's records is covered
        assert outs[name][stem + ".linkage.tsv"].decode() == want, name
        seen.add(want)
    assert len(seen) == 2
