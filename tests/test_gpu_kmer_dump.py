"""The sample's k-mer count table (bk_kmer_dump_*, `bronko call --keep-kmer-info`) against the oracle's KMC contract
(oracle.count_kmers: -k -b -ci -cs -cx on one reads file), entry for entry, sorted by k-mer."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import Params, pack_reads, synth
from tests import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def want(oracle, k, reads, **kw):
    km, ct, _ = oracle.count_kmers(k, reads, **kw)
    o = np.argsort(km, kind="stable")
    return km[o], ct[o]


def assert_dump(eng, mate, expect):
    km, ct = eng.kmer_dump(mate)
    wk, wc = expect
    assert len(km) == len(wk), (len(km), len(wk))
    assert np.array_equal(km, wk)
    assert np.array_equal(ct, wc)
    assert np.all(km[1:] > km[:-1])


@pytest.fixture(scope="module")
def hpv_index(oracle, golden_dir):
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    yield ix
    ix.close()


def test_dump_hpv_n_and_ragged_reads(oracle, hpv_index):
    reads = helpers.hpv_reads(20000, 11, with_n=True, ragged=True)
    eng = helpers.engine_from_oracle_index(hpv_index, Params())
    eng.kmer_dump_enable(16)
    helpers.hip_sample(eng, [reads], 21)
    assert_dump(eng, 0, want(oracle, 21, reads))
    eng.close()


def test_dump_parameter_edges_on_forks(oracle, hpv_index):
    reads = helpers.hpv_reads(6000, 12, with_n=True)
    parent = helpers.engine_from_oracle_index(hpv_index, Params())
    for kw in (dict(ci=1), dict(cs=5), dict(cx=40), dict(ci=2, cs=7, cx=300)):
        f = parent.fork(Params(**kw))
        f.kmer_dump_enable(12)
        helpers.hip_sample(f, [reads], 21)
        assert_dump(f, 0, want(oracle, 21, reads, **kw))
        f.close()
    parent.close()


@pytest.mark.parametrize("k", [15, 21, 31])
def test_dump_k(oracle, golden_dir, k):
    ix = oracle.Index.build(k, [os.path.join(golden_dir, "HPV16.fa")])
    reads = helpers.hpv_reads(5000, 13, with_n=True, ragged=True)
    eng = helpers.engine_from_oracle_index(ix, Params(ci=1))
    eng.kmer_dump_enable(14)
    helpers.hip_sample(eng, [reads], k)
    assert_dump(eng, 0, want(oracle, k, reads, ci=1))
    eng.close()
    ix.close()


def test_dump_paired_one_per_mate(oracle, hpv_index, golden_dir):
    g = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    gm, isnv = synth.sample_genome(g, 14)
    c1, c2 = synth.paired_codes(gm, 8000, 150, 14, isnv=isnv)
    r1, r2 = synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)
    eng = helpers.engine_from_oracle_index(hpv_index, Params())
    eng.kmer_dump_enable(14)
    helpers.hip_sample(eng, [r1, r2], 21)
    for m, reads in enumerate((r1, r2)):
        assert_dump(eng, m, want(oracle, 21, reads))
        km, _ = eng.kmer_dump(m)
        assert int(km.max()) < (1 << 42)      # (no mate bit in a key)
    eng.close()


def test_dump_growth_mid_sample(oracle, hpv_index):
    reads = helpers.hpv_reads(12000, 15, err=0.03, with_n=True)
    eng = helpers.engine_from_oracle_index(hpv_index, Params(ci=1))
    eng.kmer_dump_enable(10)
    helpers.hip_sample(eng, [reads], 21, batch=500)
    assert_dump(eng, 0, want(oracle, 21, reads, ci=1))
    eng.close()


def test_dump_all_four_push_paths(oracle, hpv_index):
    import torch
    reads = helpers.hpv_reads(6000, 16, with_n=True, ragged=True)
    expect = want(oracle, 21, reads)
    eng = helpers.engine_from_oracle_index(hpv_index, Params())
    eng.kmer_dump_enable(14)
    helpers.hip_sample(eng, [reads], 21, batch=2000)                    # packed, host
    assert_dump(eng, 0, expect)
    helpers.hip_sample(eng, [reads], 21, batch=2000, ascii_path=True)   # ASCII, host
    assert_dump(eng, 0, expect)
    words, lens = pack_reads(reads, 21)                                   # packed, device
    d_w = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    d_l = torch.from_numpy(lens.view(np.int16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.sample_begin()
    eng.push_reads_device(0, d_w.data_ptr(), words.shape[1], d_l.data_ptr(), len(lens))
    eng.sample_finish(1)
    assert_dump(eng, 0, expect)
    flat = np.frombuffer(b"".join(reads), np.uint8)                       # ASCII, device
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_flat = torch.from_numpy(flat.copy()).to("cuda:0")
    d_off = torch.from_numpy(off.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.sample_begin()
    eng.push_reads_ascii_device(0, d_flat.data_ptr(), d_off.data_ptr(), len(reads), int(off[-1]), max(len(r) for r in reads))
    eng.sample_finish(1)
    assert_dump(eng, 0, expect)
    eng.close()


def test_dump_two_samples_in_a_row(oracle, hpv_index):
    a = helpers.hpv_reads(5000, 17)
    b = helpers.hpv_reads(3000, 18, with_n=True)
    eng = helpers.engine_from_oracle_index(hpv_index, Params(ci=1))
    eng.kmer_dump_enable(12)
    helpers.hip_sample(eng, [a], 21)
    assert_dump(eng, 0, want(oracle, 21, a, ci=1))
    helpers.hip_sample(eng, [b], 21)
    assert_dump(eng, 0, want(oracle, 21, b, ci=1))
    eng.close()


def test_dump_sizes_match_full_kmer_stats(hpv_index):
    reads = helpers.hpv_reads(10000, 19, err=0.01, with_n=True)
    eng = helpers.engine_from_oracle_index(hpv_index, Params(full_kmer_stats=True, kmer_table_log2=16))
    eng.kmer_dump_enable(14)
    res = helpers.hip_sample(eng, [reads], 21)
    kept, distinct = eng.kmer_dump_size(0)
    assert kept == int(res.kmer_stats[0, 3]) and distinct == int(res.kmer_stats[0, 2]), (kept, distinct, res.kmer_stats)
    eng.close()


def test_dump_leaves_pileups_alone(hpv_index):
    reads = helpers.hpv_reads(8000, 20, with_n=True)
    off = helpers.engine_from_oracle_index(hpv_index, Params())
    on = helpers.engine_from_oracle_index(hpv_index, Params())
    on.kmer_dump_enable(14)
    a = helpers.hip_sample(off, [reads], 21)
    b = helpers.hip_sample(on, [reads], 21)
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present", "kmer_stats"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    on.kmer_dump_enable(0)                 # disabled again: the dump is no longer there
    helpers.hip_sample(on, [reads], 21)
    with pytest.raises(Exception):
        on.kmer_dump(0)
    on.close()
    off.close()


def _write_fastq_gz(path, reads, tag):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for i, r in enumerate(reads):
            f.write(b"@%s_%d\n%s\n+\n%s\n" % (tag.encode(), i, r, b"I" * len(r)))


def _counts_text(oracle, path, k=21):
    km, ct, _ = oracle.count_kmers_fastq(k, path)
    o = np.argsort(km, kind="stable")
    return "".join("%s\t%d\n" % (helpers.kmer_str(int(v), k), int(c)) for v, c in zip(km[o], ct[o])).encode()


def test_cli_keep_kmer_info_paired_fastq_gz(oracle, golden_dir, tmp_path):
    g = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    gm, isnv = synth.sample_genome(g, 1, n_snp=5, n_isnv=5)
    c1, c2 = synth.paired_codes(gm, 20000, 150, 1, isnv=isnv)
    r1, r2 = synth.codes_to_ascii(c1), synth.codes_to_ascii(c2)
    r1[7] = r1[7][:40] + b"N" + r1[7][41:]
    r2[9] = b"n" * 150
    r2[11] = r2[11].lower()
    p1, p2 = str(tmp_path / "rep1_R1.fastq.gz"), str(tmp_path / "rep1_R2.fastq.gz")
    _write_fastq_gz(p1, r1, "r1")
    _write_fastq_gz(p2, r2, "r2")
    db = os.path.join(golden_dir, "hpv.bkdb")
    outs = {}
    for flag in (True, False):
        out = str(tmp_path / ("on" if flag else "off"))
        cmd = [BRONKO, "call", "-d", db, "-1", p1, "-2", p2, "--pileup", "-o", out, "-t", "4"] + (["--keep-kmer-info"] if flag else [])
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        outs[flag] = out
    for stem, p in (("rep1_R1", p1), ("rep1_R2", p2)):
        got = open(os.path.join(outs[True], stem + "_counts.txt"), "rb").read()
        assert got == _counts_text(oracle, p), stem
    for ext in (".vcf", ".tsv"):
        assert open(os.path.join(outs[True], "rep1_R1" + ext), "rb").read() == open(os.path.join(outs[False], "rep1_R1" + ext), "rb").read()
    assert not [f for f in os.listdir(outs[False]) if f.endswith("_counts.txt")]
