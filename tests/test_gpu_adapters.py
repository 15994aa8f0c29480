"""--adapter on the GPU: adapter_find_kernel / adapter_trim_kernel behind every push path (packed records with end flags, host and
device ASCII through the *_ends_kernel variants of K0, with and without --min-base-qual), together with the primers, bk_adapter_stats,
and `bronko call --adapter` end to end.  The definition: every result equals the same run, without adapters, on the truncated reads
(the contract restated in tests/adapter_ref.py; the reads are truncated in Python) -- an engine without adapters, the host packer and
the oracle on those reads are the yardsticks, and the comparison is bit-exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import pack_reads, pack_reads_ends, synth
from bronko_amd.engine import BronkoError

from tests import adapter_ref, helpers, primer_ref
from tests.adapter_ref import seen_reads as expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
BK_ERR_INVALID, BK_ERR_STATE = -1, -5
TRUSEQ, NEXTERA = adapter_ref.PRESETS["truseq"], adapter_ref.PRESETS["nextera"]
LONG_ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"   # 33 bases: three 16-base words
ONE, THREE = [TRUSEQ], [LONG_ADAPTER, NEXTERA, TRUSEQ]


def quals_for(reads, seed):
    """Phred+33 quality lines: high mostly, a few low bases, now and then inside the adapter or the tail behind it"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        qv = rng.integers(30, 41, len(r))
        if len(r) < 1000:
            qv[rng.random(len(r)) < 0.01] = 7
        if len(r) > 40 and i % 17 == 1:
            qv[-9] = 3
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


def dataset(genome, seed, adapters, O, E, n=3000):
    """(reads, primers): library reads of a sample of the genome at 150, 32 and 300 bases, and the edge cases"""
    gm, _ = synth.sample_genome(genome, seed)
    amps = primer_ref.tile_amplicons(genome, seed)
    primers = [p for a in amps for p in a[2:]]
    reads = adapter_ref.library_reads(gm, amps, adapters, n, 150, seed + 1)
    reads += adapter_ref.library_reads(gm, amps, adapters, n // 8, 32, seed + 2) + adapter_ref.library_reads(gm, amps, adapters, n // 8, 300, seed + 3)
    reads += [r for r, _ in adapter_ref.edge_reads(genome, adapters, O, E, 150, seed + 4)]
    return reads, primers


def check(eng, res, pile, ref, ref_dump, counts, pcounts):
    helpers.assert_same_pileup(res, pile)
    assert res.kmer_stats[0].tolist() == ref.kmer_stats[0].tolist()
    for x, y in zip(eng.kmer_dump(0), ref_dump):
        assert np.array_equal(x, y)
    assert eng.adapter_stats(0) == counts
    if pcounts is not None:
        assert eng.primer_stats(0) == pcounts


def run_all_ways(eng, ix, oracle, reads, quals, adapters, O, E, k, primers=None, m=1, min_cut=0.3):
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
        want, counts, pcounts, frac = expected(reads, quals, adapters, O, E, k, min_qual, primers, m)
        # the Python counts, not the engine's (with --min-base-qual the masked bases end many a last run in front of its adapter)
        assert frac >= (min_cut if min_qual == 0 else min_cut / 2) and counts[0] > 0 and counts[1] > counts[0], (frac, counts)
        pile = oracle.sample_pileup(ix, [want])
        # the yardstick: no adapters, no primers, the host packer on the truncated (and substituted) lines
        eng.adapters_set([])
        eng.primers_set([])
        eng.sample_begin()
        w, l = pack_reads(want, k)
        eng.push_reads(0, w, l)
        ref = eng.sample_finish(1)
        ref_dump = eng.kmer_dump(0)
        helpers.assert_same_pileup(ref, pile)
        eng.adapters_set(adapters, O, E)
        if primers:
            eng.primers_set(primers, m)
        if min_qual == 0:
            # packed records with the host packer's end flags, in three batches
            w, l, e = pack_reads_ends(reads, k)
            eng.sample_begin()
            c3 = [0, len(l) // 3, len(l) // 2, len(l)]
            for a, b in zip(c3, c3[1:]):
                eng.push_reads_ends(0, w[a:b], l[a:b], e[a:b])
            check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts, pcounts)
            # ... and the same records resident on the device (they are cut in a copy: the caller's stay as they are)
            d_w = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")
            d_l = torch.from_numpy(l.view(np.int16).copy()).to("cuda:0")
            d_e = torch.from_numpy(e.copy()).to("cuda:0")
            torch.cuda.synchronize()
            eng.sample_begin()
            eng.push_reads_ends_device(0, d_w.data_ptr(), w.shape[1], d_l.data_ptr(), d_e.data_ptr(), len(l))
            check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts, pcounts)
            assert np.array_equal(d_w.cpu().numpy().view(np.uint32), w) and np.array_equal(d_l.cpu().numpy().view(np.uint16), l)
        # host lines (and qualities), in three batches
        eng.sample_begin()
        for a, b in zip(cut, cut[1:]):
            eng.push_reads_ascii(0, reads[a:b], quals[a:b] if min_qual else None, min_qual)
        check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts, pcounts)
        # device-resident lines at an odd offset (qualities at another odd offset of their own allocation)
        eng.sample_begin()
        for a, b in zip(cut, cut[1:]):
            d_off = torch.from_numpy(off[a:b + 1].copy()).to("cuda:0")
            torch.cuda.synchronize()
            longest = int((off[a + 1:b + 1] - off[a:b]).max())
            eng.push_reads_ascii_device(0, d_b.data_ptr() + 5, d_off.data_ptr(), b - a, int(off[b] - off[a]), longest,
                                        quals=d_q.data_ptr() + 3 if min_qual else None, min_qual=min_qual)
        check(eng, eng.sample_finish(1), pile, ref, ref_dump, counts, pcounts)
    eng.adapters_set([])
    eng.primers_set([])
    eng.kmer_dump_enable(0)


@pytest.mark.parametrize("adapters", [ONE, THREE], ids=["one adapter", "three adapters"])
def test_c_abi_cut_push_equals_truncated_reads_hpv(oracle, adapters):
    """HPV16, k = 21: reads of 32, 150 and 300 bases and the edge cases; O = 5, E = 0.1, and for the three adapters also O = 3 with
    E = 0.3 and O = 8 with E = 0 (the allowance staircase at its steepest and flat)."""
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    for O, E in ([(5, 0.1)] if adapters is ONE else [(5, 0.1), (3, 0.3), (8, 0.0)]):
        reads, _ = dataset(g, 40 + O, adapters, O, E)
        run_all_ways(eng, ix, oracle, reads, quals_for(reads, O), adapters, O, E, 21)
    eng.close()
    ix.close()


def test_c_abi_long_records(oracle):
    """Records of more than 20,000 bases with an adapter deep inside (a block's lanes stride over one record), an adapter behind
    which an N follows (not found), and runs longer than a record holds (cut into chunks: left as they are)."""
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    reads = [r for r, _ in adapter_ref.long_reads(g, THREE, 5)]
    cuts, _ = adapter_ref.cut_positions_all(reads, THREE, 5, 0.1)
    assert any(len(r) >= 20000 and c >= 15000 for r, c in zip(reads, cuts)) and any(len(r) > adapter_ref.MAXB and c < 0 for r, c in zip(reads, cuts))
    run_all_ways(eng, ix, oracle, reads, quals_for(reads, 1), THREE, 5, 0.1, 21)
    eng.close()
    ix.close()


@pytest.mark.parametrize("adapters", [ONE, THREE], ids=["one adapter", "three adapters"])
def test_c_abi_cut_push_equals_truncated_reads_sars_four_strains(oracle, sars_paths, adapters):
    ix = oracle.Index.build(21, sars_paths)
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(sars_paths[2])
    reads, _ = dataset(g, 91, adapters, 5, 0.1, n=4000)
    run_all_ways(eng, ix, oracle, reads, quals_for(reads, 92), adapters, 5, 0.1, 21)
    eng.close()
    ix.close()


def test_adapters_and_primers_together(oracle):
    """Truncate, then substitute: the primers see the truncated read, so the reverse-complemented primer that ends right before the
    adapter is found at the new end (asserted on the Python reference: there are such reads)."""
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    reads, primers = dataset(g, 17, THREE, 5, 0.1)
    quals = quals_for(reads, 3)
    cuts, _ = adapter_ref.cut_positions_all(reads, THREE, 5, 0.1)
    trunc, _ = adapter_ref.truncate(reads, quals, cuts)
    raw3 = primer_ref.trim_lengths_all(reads, primers, 1)[1]
    new3 = primer_ref.trim_lengths_all(trunc, primers, 1)[1]
    assert ((cuts > 0) & (raw3 == 0) & (new3 > 0)).sum() >= 50
    run_all_ways(eng, ix, oracle, reads, quals, THREE, 5, 0.1, 21, primers=primers, m=1)
    eng.close()
    ix.close()


def test_neutrality_and_errors(oracle):
    import torch
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    reads, _ = dataset(g, 7, ONE, 5, 0.1, n=1500)
    quals = [b"I" * len(r) for r in reads]
    plain = oracle.sample_pileup(ix, [reads])
    want, counts, _, _ = expected(reads, quals, ONE, 5, 0.1, 21, 0)
    cut_pile = oracle.sample_pileup(ix, [want])
    w, l, e = pack_reads_ends(reads, 21)
    # no adapters: no counters
    eng.sample_begin()
    eng.push_reads_ends(0, w, l, e)
    helpers.assert_same_pileup(eng.sample_finish(1), plain)
    with pytest.raises(BronkoError) as ei:
        eng.adapter_stats(0)
    assert ei.value.status == BK_ERR_STATE
    # adapters set, then cleared with []: the plain results again, on every path
    eng.adapters_set(ONE)
    eng.adapters_set([])
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), plain)
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21, ascii_path=True), plain)
    # what bk_adapters_set refuses, with the adapter or the parameter named
    for bad, O, E, word in (([b"AGATCGG"], 5, 0.1, "adapter 1"), ([TRUSEQ, b"A" * 65], 5, 0.1, "adapter 2"), ([TRUSEQ, b"AGATCGGAAGNGC"], 5, 0.1, "adapter 2"),
                            ([TRUSEQ] * 9, 5, 0.1, "9 adapters"), ([TRUSEQ], 2, 0.1, "min_overlap"), ([NEXTERA, TRUSEQ], 14, 0.1, "min_overlap"),
                            ([TRUSEQ], 5, -0.1, "max_error_rate"), ([TRUSEQ], 5, 0.31, "max_error_rate"), ([TRUSEQ], 5, float("nan"), "max_error_rate")):
        with pytest.raises(BronkoError) as ei:
            eng.adapters_set(bad, O, E)
        assert ei.value.status == BK_ERR_INVALID and word in str(ei.value), (bad[0], O, E, str(ei.value))
    helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), plain)   # (a refused set leaves the engine without adapters)
    # adapters set: the flag-less packed pushes are refused with a message that names adapters, so is bk_adapters_set inside a sample
    eng.adapters_set(ONE)
    eng.sample_begin()
    with pytest.raises(BronkoError) as ei:
        eng.push_reads(0, w, l)
    assert ei.value.status == BK_ERR_STATE and "adapters" in str(ei.value)
    d_w = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")
    d_l = torch.from_numpy(l.view(np.int16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(BronkoError) as ei:
        eng.push_reads_device(0, d_w.data_ptr(), w.shape[1], d_l.data_ptr(), len(l))
    assert ei.value.status == BK_ERR_STATE and "adapters" in str(ei.value)
    for arg in ([], ONE):
        with pytest.raises(BronkoError) as ei:
            eng.adapters_set(arg)
        assert ei.value.status == BK_ERR_STATE
    eng.push_reads_ends(0, w, l, e)
    res = eng.sample_finish(1)
    helpers.assert_same_pileup(res, cut_pile)
    assert eng.adapter_stats(0) == counts
    # a second sample on the same engine: the counters start again
    eng.sample_begin()
    eng.push_reads_ascii(0, reads[:500])
    eng.sample_finish(1)
    assert eng.adapter_stats(0) == expected(reads[:500], quals[:500], ONE, 5, 0.1, 21, 0)[1]
    eng.close()
    ix.close()


def test_a_fork_with_adapters_next_to_a_parent_without(oracle):
    ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    reads, _ = dataset(g, 11, THREE, 5, 0.1, n=2000)
    quals = [b"I" * len(r) for r in reads]
    fork.adapters_set(THREE)
    eng.sample_begin()
    fork.sample_begin()
    half = len(reads) // 2
    for a, b in ((0, half), (half, len(reads))):   # interleaved: both samples in flight
        eng.push_reads_ascii(0, reads[a:b])
        fork.push_reads_ascii(0, reads[a:b])
    r0, r1 = eng.sample_finish(1), fork.sample_finish(1)
    want, counts, _, _ = expected(reads, quals, THREE, 5, 0.1, 21, 0)
    helpers.assert_same_pileup(r0, oracle.sample_pileup(ix, [reads]))
    helpers.assert_same_pileup(r1, oracle.sample_pileup(ix, [want]))
    assert fork.adapter_stats(0) == counts
    with pytest.raises(BronkoError):
        eng.adapter_stats(0)
    # the parent takes another set of its own
    eng.adapters_set(ONE, 5, 0.1)
    eng.sample_begin()
    eng.push_reads_ascii(0, reads)
    want1, counts1, _, _ = expected(reads, quals, ONE, 5, 0.1, 21, 0)
    helpers.assert_same_pileup(eng.sample_finish(1), oracle.sample_pileup(ix, [want1]))
    assert eng.adapter_stats(0) == counts1 and counts1 != counts
    fork.close()
    eng.close()
    ix.close()


# ---- bronko call --adapter, end to end ----------------------------------------------------------------------------------------------
def write_fastq_gz(path, reads, quals, tag):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@%s_%d\n%s\n+\n%s\n" % (tag.encode(), i, r, q))


def call(args, out, env, timeout=600):
    res = subprocess.run([BRONKO, "call", "-d", os.path.join(helpers.GOLDEN, "hpv.bkdb")] + args + ["--pileup", "--alignment", "--keep-kmer-info",
                         "-o", out, "-t", "8"], capture_output=True, text=True, env=env, timeout=timeout)
    assert res.returncode == 0, res.stdout + res.stderr
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, res.stdout + res.stderr


@pytest.mark.parametrize("inflate", ["one thread", "several threads"])
def test_call_adapter_equals_a_call_on_truncated_files(tmp_path, inflate):
    """Every output (VCFs, pileup TSVs, overview, .mfa, _counts.txt) of `--adapter truseq` is byte-identical to a plain call on the
    truncated files (same basenames, another directory): three paired samples and, in a call of its own, a single-end one; with and
    without --primers; once more with --min-base-qual 20 and a second adapter.  One inflate thread: the line loop and K0's
    *_ends_kernel variants; several: the host packer's end flags."""
    g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
    amps = primer_ref.tile_amplicons(g, 3)
    primers = [p for a in amps for p in a[2:]]
    pfile = str(tmp_path / "primers.fa")
    open(pfile, "w").write("".join(">p%d\n%s\n" % (i, p.decode()) for i, p in enumerate(primers)))
    samples = []
    for i in range(3):
        gm, _ = synth.sample_genome(g, 20 + i, n_snp=5, n_isnv=0)
        mates = []
        for m in range(2):
            r = adapter_ref.library_reads(gm, amps, [TRUSEQ, TRUSEQ, TRUSEQ, NEXTERA], 6000, 150, 100 + 2 * i + m)
            r += [x for x, _ in adapter_ref.edge_reads(g, [TRUSEQ, NEXTERA], 5, 0.1, 150, 7 + m)]
            mates.append((r, quals_for(r, 200 + 2 * i + m)))
        samples.append(mates)
    env = dict(os.environ)
    if inflate == "one thread":
        env["BRONKO_INFLATE_THREADS"] = "1"

    def files(name, adapters, O, E, min_qual):
        d = tmp_path / name
        d.mkdir()
        for i, mates in enumerate(samples):
            for m, (r, q) in enumerate(mates):
                if adapters:
                    cuts, _ = adapter_ref.cut_positions_all(r, adapters, O, E, q, min_qual)
                    assert (cuts >= 0).mean() >= 0.3 and (cuts == 0).sum() >= 1   # (some reads are written as N / !)
                    r, q = adapter_ref.truncate(r, q, cuts)
                write_fastq_gz(str(d / ("s%d_R%d.fastq.gz" % (i, m + 1))), r, q, "ab"[m])
        return str(d)
    pairs = lambda d: (["-1"] + [os.path.join(d, "s%d_R1.fastq.gz" % i) for i in range(3)] + ["-2"] + [os.path.join(d, "s%d_R2.fastq.gz" % i) for i in range(3)])
    single = lambda d: ["-r", os.path.join(d, "s1_R2.fastq.gz")]
    orig = files("orig", None, 0, 0, 0)
    n_out = 0
    for tag, flags, adapters, O, E, min_qual in (("a", ["--adapter", "truseq"], [TRUSEQ], 5, 0.1, 0),
                                                 ("b", ["--adapter", "truseq", "nextera", "--adapter-min-overlap", "4", "--adapter-error-rate", "0.2",
                                                        "--min-base-qual", "20"], [TRUSEQ, NEXTERA], 4, 0.2, 20)):
        want_dir = files("trunc_" + tag, adapters, O, E, min_qual)
        rest = ["--min-base-qual", "20"] if min_qual else []
        for inputs in (pairs, single):
            for with_primers in ([], ["--primers", pfile]):
                n_out += 1
                got, log = call(inputs(orig) + flags + with_primers + ["--verbose"], str(tmp_path / ("o_got%d" % n_out)), env)
                want, _ = call(inputs(want_dir) + rest + with_primers, str(tmp_path / ("o_want%d" % n_out)), env)
                assert sorted(got) == sorted(want)
                assert any(n.endswith("_counts.txt") for n in got) and any(n.endswith(".vcf") for n in got), sorted(got)
                assert inputs is single or any(n.endswith(".mfa") for n in got), sorted(got)   # (an alignment takes three samples)
                for n in got:
                    assert got[n].replace(orig.encode(), b"DIR") == want[n].replace(want_dir.encode(), b"DIR"), (tag, n)
                # --verbose: one line per reads file with the two counters
                for i, mates in enumerate(samples):
                    for m, (r, q) in enumerate(mates):
                        if inputs is single and (i, m) != (1, 1):
                            continue
                        cuts, s1 = adapter_ref.cut_positions_all(r, adapters, O, E, q, min_qual)
                        c = adapter_ref.record_counts(r, cuts, s1, 21)
                        line = "adapters: %d reads cut, %d bases removed in %s" % (c[0], c[1], os.path.join(orig, "s%d_R%d.fastq.gz" % (i, m + 1)))
                        assert line in log, line
    # and cutting matters: without --adapter the same files give other counts
    plain, _ = call(single(orig), str(tmp_path / "o_plain"), env)
    name = next(n for n in got if n.endswith("_counts.txt"))
    assert plain[name] != got[name]
