"""Every optional pass of a sample on one engine in one sample: full_kmer_stats, the k-mer dump, indels, linkage, a primer and an
adapter set, and behind the pileup the calls, the consensus and the region depths.  Each of them adds work to bk_sample_begin, to
every push and to the sample's end; the other tests enable them one or two at a time.

Every download of the engine that has them all must equal, exactly, what six engines with one extra each give for the same reads --
all results are integers or copies, so there is no tolerance.  The primer and the adapter set change the records themselves, so
every engine has them (test_gpu_linkage.py::test_with_primers_and_adapters_set's); the six engines are: nothing more (the pileup, the
statistics, the trimming counters, the calls, the noise, the consensus), full_kmer_stats, the k-mer dump, regions, indels, linkage.
The reads are tests.linkage_cases.Planted's, a third of them cut short by the adapter.  The sample is pushed in two batches, packed and then ASCII: the passes behind the scan take the record count from the host for the
first and from the device for the second.  A second sample on the engine with everything covers what bk_sample_begin clears."""
import os

import numpy as np
import pytest

from bronko_amd import Params, pack_reads_ends
from bronko_amd.hostlib import HostIndex
from tests import linkage_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 21
TRUSEQ = b"AGATCGGAAGAGC"
CUT = 777                            # the packed batch's reads; the rest are pushed as ASCII
EXTRAS = ("full_kmer_stats", "kmer_dump", "regions", "indels", "linkage")


def _engine(ix, primers, extras):
    eng = ix.engine(Params(full_kmer_stats="full_kmer_stats" in extras, kmer_table_log2=16))   # (small tables: both grow in the sample)
    eng.adapters_set([TRUSEQ], 5, 0.1)
    eng.primers_set(primers, 1)
    if "kmer_dump" in extras:
        eng.kmer_dump_enable(16)
    if "indels" in extras:
        eng.indels_enable()
    if "linkage" in extras:
        eng.linkage_enable(8, 100)    # (a row store that grows in the sample)
    if "regions" in extras:
        eng.regions_set([(0, 0, s, s + 400) for s in range(0, 7600, 400)] + [(0, 0, 100, 7100)])
    return eng


def _fields(st):
    """A ctypes structure's fields but its padding, which nothing writes; a double as its bits"""
    vals = [(name, getattr(st, name)) for name, _ in st._fields_ if name != "pad"]
    return tuple((name, v.hex() if isinstance(v, float) else v) for name, v in vals)


def _sample(eng, reads, sites, extras, common):
    """One sample; every download that the extras give (common: and those that every engine gives), as values that compare exactly"""
    w, l, e = pack_reads_ends(reads[:CUT], K)
    eng.sample_begin()
    eng.push_reads_ends(0, w, l, e)
    eng.push_reads_ascii(0, reads[CUT:])
    res = eng.sample_finish(1)
    got = {}
    if common:
        got.update(zip(("fwd_depth", "rev_depth", "fwd_nk", "rev_nk"), (a.tobytes() for a in res.arrays())))
        got["stats"], got["present"] = res.stats.tolist(), res.present.tolist()
        got["primer_stats"], got["adapter_stats"] = eng.primer_stats(0), eng.adapter_stats(0)
    if "full_kmer_stats" in extras:
        got["kmer_stats"] = res.kmer_stats.tolist()
    if "kmer_dump" in extras:
        got["kmer_dump_size"] = eng.kmer_dump_size(0)
        got["kmer_dump"] = tuple(a.tobytes() for a in eng.kmer_dump(0))
    if common or "regions" in extras:
        eng.sample_call(1, eng.call_params(min_depth=10))
    if common:
        summ, recs = eng.download_calls()
        got["calls"] = (_fields(summ), [_fields(r) for r in recs])
        got["noise"] = eng.download_noise().tobytes()
        eng.sample_consensus()
        summ, letters = eng.download_consensus()
        got["consensus"] = (_fields(summ), letters)
    if "regions" in extras:
        eng.sample_region_depths(10)
        summ, rows = eng.download_region_depths()
        got["regions"] = (_fields(summ), rows)
    if "indels" in extras:
        eng.sample_indels(1, 0)
        summ, rows = eng.download_indels()
        got["indels"] = (_fields(summ), rows, eng.download_indel_span().tobytes())
    if "linkage" in extras:
        got["link_rows"] = eng.download_link_rows()
        eng.sample_linkage(sites, 1000)
        summ, pairs = eng.download_linkage()
        got["linkage"] = (_fields(summ), pairs)
    return got


def test_all_extras_equal_each_alone():
    planted = linkage_cases.Planted(K)
    rng = np.random.default_rng(5)
    reads = []
    for i, r in enumerate(planted.reads):                        # a third of the reads run into the adapter and a tail, as in
        r = r.encode() if isinstance(r, str) else bytes(r)       # test_gpu_linkage.py::test_with_primers_and_adapters_set
        if i % 3 == 0:
            r = (r[:int(rng.integers(60, 150))] + TRUSEQ + b"G" * 150)[:150]
        reads.append(r)
    primers = [planted.g.text[p:p + 22].encode() for p in range(1720, 3700, 97)]
    ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
    want = {}
    try:
        for extras in [()] + [(x,) for x in EXTRAS]:
            eng = _engine(ix, primers, extras)
            try:
                want.update(_sample(eng, reads, planted.sites, extras, extras == ()))
            finally:
                eng.close()
        # (the sample is not an empty one: reads were trimmed, placed, called and counted)
        assert want["primer_stats"][0] > 0 and want["adapter_stats"][0] > 200 and len(want["link_rows"]) > 1000 and len(want["linkage"][1]) > 0
        assert dict(want["indels"][0])["anchored"] > 1000 and dict(want["indels"][0])["ref_spanning"] > 1000
        assert len(want["kmer_dump"][0]) > 8 * 1000 and len(want["regions"][1]) == 20 and len(want["consensus"][1]) > 7000
        eng = _engine(ix, primers, EXTRAS)
        try:
            for sample in (1, 2):
                got = _sample(eng, reads, planted.sites, EXTRAS, True)
                assert got.keys() == want.keys()
                for name in want:
                    assert got[name] == want[name], (sample, name)
        finally:
            eng.close()
    finally:
        ix.close()
