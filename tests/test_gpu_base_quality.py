"""--min-base-qual on the GPU: the quality-aware twins of K0 (pack_words_qual_kernel, pack_slow_qual_kernel) behind
bk_push_reads_ascii_qual / _device, and `bronko call --min-base-qual` end to end.  The definition: every result equals the same run
on the reads with each base whose quality byte is below '!' + Q replaced by N -- the existing host packer and the oracle on those
reads are the yardsticks."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import pack_reads, synth
from bronko_amd.engine import BronkoError

from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def quals_for(reads, seed, p_low=0.04):
    """Phred+33 quality lines: 30..40 mostly, a few low ones, and the packer's word boundaries (15/16/31/32) masked now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        qv = rng.integers(30, 41, len(r))
        qv[rng.random(len(r)) < p_low] = rng.integers(0, 20)
        if i % 9 == 1:
            qv[[p for p in (15, 16, 31, 32) if p < len(r)]] = 2
        elif i % 9 == 2:
            qv[:] = 5                               # the whole read
        elif i % 9 == 3:
            qv[:] = 40                              # nothing
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


def masked(reads, quals, q):
    out = []
    for r, ql in zip(reads, quals):
        a = np.frombuffer(r, np.uint8).copy()
        a[np.frombuffer(ql, np.uint8) < 33 + q] = ord("N")
        out.append(a.tobytes())
    return out


def reads_of(genome, n, read_len, seed):
    gm, isnv = synth.sample_genome(genome, seed)
    reads = synth.codes_to_ascii(synth.single_end_codes(gm, n, read_len, seed + 1, err=0.01, isnv=isnv))
    r = np.random.default_rng(seed)
    out = []
    for i, rd in enumerate(reads):   # lower case and N now and then, and ragged lengths
        if i % 17 == 4:
            rd = rd.lower()
        if i % 23 == 5:
            rd = rd[:10] + b"N" + rd[11:]
        if i % 5 == 0:
            rd = rd[: int(r.integers(0, len(rd) + 1))]
        out.append(rd)
    return out


def run_all_ways(eng, ix, oracle, reads, quals, k, q):
    import torch
    want = masked(reads, quals, q)
    pile = oracle.sample_pileup(ix, [want])
    # the yardstick: the host packer on the N-substituted lines
    eng.kmer_dump_enable()
    eng.sample_begin()
    w, l = pack_reads(want, k)
    eng.push_reads(0, w, l)
    ref = eng.sample_finish(1)
    ref_dump = eng.kmer_dump(0)
    helpers.assert_same_pileup(ref, pile)
    # host lines + qualities, in three batches
    eng.sample_begin()
    cut = [0, len(reads) // 3, len(reads) // 2, len(reads)]
    for a, b in zip(cut, cut[1:]):
        eng.push_reads_ascii(0, reads[a:b], quals[a:b], q)
    got = eng.sample_finish(1)
    helpers.assert_same_pileup(got, pile)
    assert got.kmer_stats[0].tolist() == ref.kmer_stats[0].tolist()
    for x, y in zip(eng.kmer_dump(0), ref_dump):
        assert np.array_equal(x, y)
    # device-resident lines at an odd offset, qualities at another odd offset of their own allocation
    flat = np.frombuffer(b"".join(reads), np.uint8)
    qflat = np.frombuffer(b"".join(quals), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_b = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda:0")
    d_q = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda:0")
    d_b[5:5 + len(flat)] = torch.from_numpy(flat.copy()).to("cuda:0")
    d_q[3:3 + len(flat)] = torch.from_numpy(qflat.copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.sample_begin()
    for a, b in zip(cut, cut[1:]):
        d_off = torch.from_numpy(off[a:b + 1].copy()).to("cuda:0")
        torch.cuda.synchronize()
        longest = int((off[a + 1:b + 1] - off[a:b]).max())
        eng.push_reads_ascii_device(0, d_b.data_ptr() + 5, d_off.data_ptr(), b - a, int(off[b] - off[a]), longest,
                                    quals=d_q.data_ptr() + 3, min_qual=q)
    got = eng.sample_finish(1)
    helpers.assert_same_pileup(got, pile)
    assert got.kmer_stats[0].tolist() == ref.kmer_stats[0].tolist()
    for x, y in zip(eng.kmer_dump(0), ref_dump):
        assert np.array_equal(x, y)
    eng.kmer_dump_enable(0)
    return got


@pytest.mark.parametrize("read_len", [32, 150, 300])
def test_c_abi_masked_push_equals_n_substituted_reads_hpv(oracle, read_len):
    """HPV16, k = 21: reads of up to 32 bases (two-word records), 150, and 300 (records longer than 256 bases: pack_slow_qual_kernel)."""
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    reads = reads_of(g, 6000, read_len, 31 + read_len)
    quals = quals_for(reads, read_len)
    for q in (20, 35):
        run_all_ways(eng, ix, oracle, reads, quals, 21, q)
    # min_qual 0 is the plain call; a value out of range is refused
    eng.sample_begin()
    eng.push_reads_ascii(0, reads, quals, 0)
    res = eng.sample_finish(1)
    helpers.assert_same_pileup(res, oracle.sample_pileup(ix, [reads]))
    eng.sample_begin()
    with pytest.raises(BronkoError):
        eng.push_reads_ascii(0, reads, quals, 94)
    eng.sample_finish(1)
    eng.close()
    ix.close()


def test_c_abi_masked_push_equals_n_substituted_reads_sars_four_strains(oracle, sars_paths):
    ix = oracle.Index.build(21, sars_paths)
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(sars_paths[2])
    reads = reads_of(g, 8000, 150, 77)
    quals = quals_for(reads, 78)
    run_all_ways(eng, ix, oracle, reads, quals, 21, 20)
    eng.close()
    ix.close()


# ---- bronko call --min-base-qual, end to end ------------------------------------------------------------------------------------
def sequenced_pairs(n_pairs, seed):
    """HPV16 pairs with realistic quality strings: 1 % sequencing errors, most of them (and a few correct bases) at low quality"""
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    gm, isnv = synth.sample_genome(g, seed, n_snp=5, n_isnv=8)
    c1, c2 = synth.paired_codes(gm, n_pairs, 150, seed, err=0.0, isnv=isnv)
    rng = np.random.default_rng(seed)
    out = []
    for c in (c1, c2):
        c = np.array(c, np.uint8)
        qv = rng.integers(28, 41, c.shape)
        err = rng.random(c.shape) < 0.01
        c[err] = (c[err] + rng.integers(1, 4, int(err.sum()))) & 3
        low = err & (rng.random(c.shape) < 0.85)
        qv[low] = rng.integers(2, 15, int(low.sum()))
        stray = rng.random(c.shape) < 0.003
        qv[stray] = rng.integers(5, 19, int(stray.sum()))
        out.append((synth.codes_to_ascii(c), [(x + 33).astype(np.uint8).tobytes() for x in qv]))
    return out


def write_fastq_gz(path, reads, quals, tag):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@%s_%d\n%s\n+\n%s\n" % (tag.encode(), i, r, q))


def call(args, out, env, timeout=600):
    res = subprocess.run([BRONKO, "call", "-d", os.path.join(helpers.GOLDEN, "hpv.bkdb")] + args + ["--pileup", "--alignment", "--keep-kmer-info",
                         "-o", out, "-t", "8"], capture_output=True, text=True, env=env, timeout=timeout)
    assert res.returncode == 0, res.stdout + res.stderr
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}


@pytest.mark.parametrize("inflate", ["one thread", "several threads"])
def test_call_min_base_qual_equals_a_call_on_n_substituted_files(tmp_path, inflate):
    """Every output (VCFs, pileup TSVs, overview, .mfa, _counts.txt) of `--min-base-qual 20` on three paired samples is
    byte-identical to a plain call on the same files with the low-quality bases replaced by N (same basenames, another directory).
    One inflate thread: the line loop and the GPU twin of K0; several: the host packer with its record carry."""
    samples = [sequenced_pairs(15000, 5 + i) for i in range(3)]   # (--alignment needs three samples)
    dirs = {}
    for name in ("orig", "masked"):
        d = tmp_path / name
        d.mkdir()
        for i, ((r1, q1), (r2, q2)) in enumerate(samples):
            if name == "masked":
                r1, r2 = masked(r1, q1, 20), masked(r2, q2, 20)
            write_fastq_gz(str(d / ("s%d_R1.fastq.gz" % i)), r1, q1, "a")
            write_fastq_gz(str(d / ("s%d_R2.fastq.gz" % i)), r2, q2, "b")
        dirs[name] = str(d)
    env = dict(os.environ)
    if inflate == "one thread":
        env["BRONKO_INFLATE_THREADS"] = "1"
    pairs = lambda d: (["-1"] + [os.path.join(d, "s%d_R1.fastq.gz" % i) for i in range(3)] +
                       ["-2"] + [os.path.join(d, "s%d_R2.fastq.gz" % i) for i in range(3)])
    got = call(pairs(dirs["orig"]) + ["--min-base-qual", "20"], str(tmp_path / "o_q"), env)
    want = call(pairs(dirs["masked"]), str(tmp_path / "o_m"), env)
    assert sorted(got) == sorted(want)
    assert any(n.endswith("_counts.txt") for n in got) and any(n.endswith(".mfa") for n in got), sorted(got)
    for n in got:
        assert got[n].replace(dirs["orig"].encode(), b"DIR") == want[n].replace(dirs["masked"].encode(), b"DIR"), n
    # masking changes something: without it the sequencing errors give more variant k-mers (what the noise estimate is made of)
    # or more minor variants
    plain = call(pairs(dirs["orig"]), str(tmp_path / "o_p"), env)
    rows = lambda o: [ln.split("\t") for ln in o["bronko_overview.tsv"].decode().splitlines()[1:]]
    for m, p in zip(rows(got), rows(plain)):
        assert int(m[3]) < int(p[3]) or int(m[7]) < int(p[7]), (m, p)
