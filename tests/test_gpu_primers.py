"""--primers on the GPU: primer_trim_kernel behind every push path (packed records with end flags, host and device ASCII through the
*_ends_kernel variants of K0, with and without --min-base-qual), bk_primer_stats, and `bronko call --primers` end to end.  The
definition: every result equals the same run, without primers, on the reads with the primer letters replaced by N (the contract
restated in tests/primer_ref.py) -- an engine without primers, the host packer and the oracle on those reads are the yardsticks."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import pack_reads, pack_reads_ends, synth
from bronko_amd.engine import BronkoError

from tests import helpers, primer_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
BK_ERR_INVALID, BK_ERR_STATE = -1, -5


def quals_for(reads, seed):
    """Phred+33 quality lines: high mostly, a few low bases, now and then inside the primer stretch or at a read's end"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        qv = rng.integers(30, 41, len(r))
        qv[rng.random(len(r)) < 0.02] = 7
        if len(r) > 20:
            if i % 13 == 1:
                qv[8] = 3            # inside the 5' primer: interrupted, no match
            elif i % 13 == 2:
                qv[-5] = 3           # inside the 3' primer
            elif i % 13 == 3:
                qv[0] = 3            # the first letter: the 5' run starts behind it
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


def dataset(genome, seed, read_len, n=5000):
    """(primers, reads): amplicon and shotgun reads of a sample of the genome, the edge cases, and reads of 32 and 300 bases"""
    gm, _ = synth.sample_genome(genome, seed)
    amps = primer_ref.tile_amplicons(genome, seed)
    primers = [p for a in amps for p in a[2:]]
    assert {12, 31, 32, 33, 64} <= {len(p) for p in primers} and len(primers) <= 1024
    reads = primer_ref.amplicon_reads(genome, gm, amps, n, read_len, seed + 1)
    reads += primer_ref.edge_reads(genome, amps, read_len)
    if read_len == 150:
        reads += primer_ref.amplicon_reads(genome, gm, amps, 300, 32, seed + 2) + primer_ref.amplicon_reads(genome, gm, amps, 300, 300, seed + 3)
    else:
        reads = [r[:read_len] for r in reads]
    return primers, reads


def check(eng, res, pile, ref, ref_dump, counts):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[0].tolist() == ref.kmer_stats[0].tolist()
    for x, y in zip(eng.kmer_dump(0), ref_dump):
        assert np.array_equal(x, y)
    assert eng.primer_stats(0) == counts


def run_all_ways(eng, ix, oracle, reads, quals, primers, k, m, exercise=False):
    import torch
    cut = [0, len(reads) // 3, len(reads) // 2, len(reads)]
    flat = np.frombuffer(b"".join(reads), np.uint8)
    qflat = np.frombuffer(b"".join(quals), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_b = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda:0")
    d_q = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda:0")
    d_b[5:5 + len(flat)] = torch.from_numpy(flat.copy()).to("cuda:0")
    d_q[3:3 + len(flat)] = torch.from_numpy(qflat.copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.kmer_dump_enable()
    for min_qual in (0, 20):
        p5, p3, e0, s1 = primer_ref.trim_lengths_all(reads, primers, m, quals, min_qual)
        if exercise and min_qual == 0:   # the test exercises the feature (the Python counts, not the engine's)
            whole = sum(1 for r, a, b, e in zip(reads, p5, p3, e0) if len(r) and e == len(r) and a + b >= len(r))
            assert (p5 > 0).mean() >= 0.6 and (p3 > 0).mean() >= 0.1 and whole >= 1, ((p5 > 0).mean(), (p3 > 0).mean(), whole)
        base = reads
        if min_qual:
            base = []
            for r, ql in zip(reads, quals):
                a = np.frombuffer(r, np.uint8).copy()
                a[np.frombuffer(ql, np.uint8) < 33 + min_qual] = ord("N")
                base.append(a.tobytes())
        want = primer_ref.substitute(base, p5, p3, e0)
        counts = primer_ref.record_counts(reads, p5, p3, e0, s1, k)
        assert min_qual or counts[0] > 0
        pile = oracle.sample_pileup(ix, [want])
        # the yardstick: no primers, the host packer on the N-substituted lines
        eng.primers_set([])
        eng.sample_begin()
        w, l = pack_reads(want, k)
        eng.push_reads(0, w, l)
        ref = eng.sample_finish(1)
        ref_dump = eng.kmer_dump(0)
        helpers.assert_same_pileup(ref, pile)
        eng.primers_set(primers, m)
        if min_qual == 0:
            # packed records with the host packer's end flags, in three batches
            w, l, e = pack_reads_ends(reads, k)
            eng.sample_begin()
            c3 = [0, len(l) // 3, len(l) // 2, len(l)]
            for a, b in zip(c3, c3[1:]):
                eng.push_reads_ends(0, w[a:b], l[a:b], e[a:b])
            check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts)
            # ... and the same records resident on the device (they are trimmed in a copy: the caller's stay as they are)
            d_w = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")
            d_l = torch.from_numpy(l.view(np.int16).copy()).to("cuda:0")
            d_e = torch.from_numpy(e.copy()).to("cuda:0")
            torch.cuda.synchronize()
            eng.sample_begin()
            eng.push_reads_ends_device(0, d_w.data_ptr(), w.shape[1], d_l.data_ptr(), d_e.data_ptr(), len(l))
            check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts)
            assert np.array_equal(d_w.cpu().numpy().view(np.uint32), w) and np.array_equal(d_l.cpu().numpy().view(np.uint16), l)
        # host lines (and qualities), in three batches
        eng.sample_begin()
        for a, b in zip(cut, cut[1:]):
            eng.push_reads_ascii(0, reads[a:b], quals[a:b] if min_qual else None, min_qual)
        check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts)
        # device-resident lines at an odd offset (qualities at another odd offset of their own allocation)
        eng.sample_begin()
        for a, b in zip(cut, cut[1:]):
            d_off = torch.from_numpy(off[a:b + 1].copy()).to("cuda:0")
            torch.cuda.synchronize()
            longest = int((off[a + 1:b + 1] - off[a:b]).max())
            eng.push_reads_ascii_device(0, d_b.data_ptr() + 5, d_off.data_ptr(), b - a, int(off[b] - off[a]), longest,
                                        quals=d_q.data_ptr() + 3 if min_qual else None, min_qual=min_qual)
        check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts)
    eng.primers_set([])
    eng.kmer_dump_enable(0)


@pytest.mark.parametrize("read_len", [32, 150, 300])
def test_c_abi_trimmed_push_equals_n_substituted_reads_hpv(oracle, read_len):
    """HPV16, k = 21: reads cut to 32 bases (two-word records), the mixed set around 150, and reads of up to 300 (records longer than
    256 bases: pack_slow_*_ends_kernel); M = 0, 1 and 3."""
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    primers, reads = dataset(g, 40 + read_len, read_len)
    quals = quals_for(reads, read_len)
    for m in (0, 1, 3):
        run_all_ways(eng, ix, oracle, reads, quals, primers, 21, m, exercise=(m == 1 and read_len == 150))
    eng.close()
    ix.close()


def test_c_abi_trimmed_push_equals_n_substituted_reads_sars_four_strains(oracle, sars_paths):
    ix = oracle.Index.build(21, sars_paths)
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(sars_paths[2])
    primers, reads = dataset(g, 91, 150, n=7000)
    assert 150 <= len(primers) <= 1024
    quals = quals_for(reads, 92)
    for m in (0, 1, 3):
        run_all_ways(eng, ix, oracle, reads, quals, primers, 21, m, exercise=(m == 1))
    eng.close()
    ix.close()


def test_neutrality_and_errors(oracle):
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    primers, reads = dataset(g, 7, 150, n=2000)
    plain = oracle.sample_pileup(ix, [reads])
    w, l, e = pack_reads_ends(reads, 21)
    # no primers: the _ends push is the plain one; no counters
    eng.sample_begin()
    eng.push_reads_ends(0, w, l, e)
    helpers.assert_same_pileup(eng.sample_finish(1), plain)
    with pytest.raises(BronkoError) as ei:
        eng.primer_stats(0)
    assert ei.value.status == BK_ERR_STATE
    # primers set, then cleared: the plain results again
    eng.primers_set(primers, 1)
    eng.primers_set([])
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), plain)
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21, ascii_path=True), plain)
    # bad primers
    for bad, m in (([b"ACGTACGTACG"], 1), ([b"A" * 65], 1), ([b"ACGTACGTACGTNACGT"], 1), ([b"ACGTACGTACGTACGT"], 4), ([b"ACGTACGTACGTACGT"], -1),
                   ([b"ACGTACGTACGTACGT"] * 1025, 1)):
        with pytest.raises(BronkoError) as ei:
            eng.primers_set(bad, m)
        assert ei.value.status == BK_ERR_INVALID, (bad[0], m)
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), plain)   # (a refused set leaves the engine without primers)
    # primers set: the flag-less packed pushes are refused, bk_primers_set inside a sample is refused
    import torch
    eng.primers_set(primers, 1)
    eng.sample_begin()
    with pytest.raises(BronkoError) as ei:
        eng.push_reads(0, w, l)
    assert ei.value.status == BK_ERR_STATE
    d_w = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")
    d_l = torch.from_numpy(l.view(np.int16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(BronkoError) as ei:
        eng.push_reads_device(0, d_w.data_ptr(), w.shape[1], d_l.data_ptr(), len(l))
    assert ei.value.status == BK_ERR_STATE
    with pytest.raises(BronkoError) as ei:
        eng.primers_set([])
    assert ei.value.status == BK_ERR_STATE
    eng.push_reads_ends(0, w, l, e)
    res = eng.sample_finish(1)
    helpers.assert_same_pileup(res, oracle.sample_pileup(ix, [primer_ref.trimmed(reads, primers, 1)]))
    eng.close()
    ix.close()


def test_a_fork_with_primers_next_to_a_parent_without(oracle):
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    primers, reads = dataset(g, 11, 150, n=3000)
    fork.primers_set(primers, 1)
    eng.sample_begin()
    fork.sample_begin()
    half = len(reads) // 2
    for a, b in ((0, half), (half, len(reads))):   # interleaved: both samples in flight
        eng.push_reads_ascii(0, reads[a:b])
        fork.push_reads_ascii(0, reads[a:b])
    r0, r1 = eng.sample_finish(1), fork.sample_finish(1)
    helpers.assert_same_pileup(r0, oracle.sample_pileup(ix, [reads]))
    helpers.assert_same_pileup(r1, oracle.sample_pileup(ix, [primer_ref.trimmed(reads, primers, 1)]))
    p5, p3, e0, s1 = primer_ref.trim_lengths_all(reads, primers, 1)
    assert fork.primer_stats(0) == primer_ref.record_counts(reads, p5, p3, e0, s1, 21)
    fork.close()
    eng.close()
    ix.close()


# ---- bronko call --primers, end to end ----------------------------------------------------------------------------------------------
def write_fastq_gz(path, reads, quals, tag):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@%s_%d\n%s\n+\n%s\n" % (tag.encode(), i, r, q))


def call(args, out, env, timeout=600):
    res = subprocess.run([BRONKO, "call", "-d", os.path.join(helpers.GOLDEN, "hpv.bkdb")] + args + ["--pileup", "--alignment", "--keep-kmer-info",
                         "-o", out, "-t", "8"], capture_output=True, text=True, env=env, timeout=timeout)
    assert res.returncode == 0, res.stdout + res.stderr
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, res.stdout + res.stderr


def vcf_af(vcf, pos):
    for ln in vcf.decode().splitlines():
        f = ln.split("\t")
        if not ln.startswith("#") and int(f[1]) == pos:
            return float(f[7].split("AF=")[1].split(";")[0])
    return None


@pytest.mark.parametrize("inflate", ["one thread", "several threads"])
def test_call_primers_equals_a_call_on_n_substituted_files(tmp_path, inflate):
    """Every output (VCFs, pileup TSVs, overview, .mfa, _counts.txt) of `--primers` on three paired samples is byte-identical to a
    plain call on the same files with the primer letters replaced by N (same basenames, another directory); once more together with
    --min-base-qual 20.  One inflate thread: the line loop and K0's *_ends_kernel variants; several: the host packer's end flags.
    And trimming matters: a SNV of the sample under a primer site, covered by the neighbouring amplicon's interior, is diluted by
    the primer's reference base without --primers."""
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    amps = primer_ref.tile_amplicons(g, 3)
    primers = [p for a in amps for p in a[2:]]
    # the planted SNV: under the forward primer of an amplicon whose left neighbour is a long one
    j = next(i for i in range(2, len(amps)) if amps[i - 1][1] - amps[i - 1][0] > 200 and amps[i - 1][1] - amps[i][0] >= 60 and len(amps[i][2]) >= 18)
    snv = amps[j][0] + 5
    assert amps[j - 1][1] - len(amps[j - 1][3]) > snv + 21   # (inside the neighbour, clear of its reverse primer by more than k)
    pfile = str(tmp_path / "primers.fa")
    open(pfile, "w").write("".join(">p%d\n%s\n" % (i, p.decode()) for i, p in enumerate(primers)))
    samples = []
    for i in range(3):
        gm, _ = synth.sample_genome(g, 20 + i, n_snp=5, n_isnv=0)
        gm = bytearray(gm)
        gm[snv] = b"ACGT"[(b"ACGT".index(bytes([g[snv]])) + 1) & 3]
        mates = []
        for m in range(2):
            r = primer_ref.amplicon_reads(g, bytes(gm), amps, 15000, 150, 100 + 2 * i + m) + primer_ref.edge_reads(g, amps, 150)
            r = [x for x in r if x]
            mates.append((r, quals_for(r, 200 + 2 * i + m)))
        samples.append(mates)
    env = dict(os.environ)
    if inflate == "one thread":
        env["BRONKO_INFLATE_THREADS"] = "1"

    def files(name, min_qual):
        d = tmp_path / name
        d.mkdir()
        for i, mates in enumerate(samples):
            for m, (r, q) in enumerate(mates):
                if name.startswith("trim"):
                    r = primer_ref.trimmed(r, primers, 1, q, min_qual)
                write_fastq_gz(str(d / ("s%d_R%d.fastq.gz" % (i, m + 1))), r, q, "ab"[m])
        return str(d)
    pairs = lambda d: (["-1"] + [os.path.join(d, "s%d_R1.fastq.gz" % i) for i in range(3)] +
                       ["-2"] + [os.path.join(d, "s%d_R2.fastq.gz" % i) for i in range(3)])
    orig = files("orig", 0)
    for min_qual in (0, 20):
        extra = ["--min-base-qual", "20"] if min_qual else []
        want_dir = files("trim%d" % min_qual, min_qual)
        got, log = call(pairs(orig) + ["--primers", pfile, "--verbose"] + extra, str(tmp_path / ("o_p%d" % min_qual)), env)
        want, _ = call(pairs(want_dir) + extra, str(tmp_path / ("o_t%d" % min_qual)), env)
        assert sorted(got) == sorted(want)
        assert any(n.endswith("_counts.txt") for n in got) and any(n.endswith(".mfa") for n in got), sorted(got)
        for n in got:
            assert got[n].replace(orig.encode(), b"DIR") == want[n].replace(want_dir.encode(), b"DIR"), n
        # --verbose: one line per reads file with the three counters
        for i, mates in enumerate(samples):
            for m, (r, q) in enumerate(mates):
                p5, p3, e0, s1 = primer_ref.trim_lengths_all(r, primers, 1, q, min_qual)
                c = primer_ref.record_counts(r, p5, p3, e0, s1, 21)
                line = "primers: %d reads trimmed at the 5' end, %d at the 3' end, %d bases masked in %s" % (
                    c[0], c[1], c[2], os.path.join(orig, "s%d_R%d.fastq.gz" % (i, m + 1)))
                assert line in log, line
        if min_qual == 0:
            plain, _ = call(pairs(orig), str(tmp_path / "o_plain"), env)
            for i in range(3):
                with_p, without = vcf_af(got["s%d_R1.vcf" % i], snv + 1), vcf_af(plain["s%d_R1.vcf" % i], snv + 1)
                assert with_p is not None and (without is None or with_p > without), (i, with_p, without)
