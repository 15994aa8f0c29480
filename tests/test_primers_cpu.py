"""--primers on the host (no GPU): the end flags the packers give their records -- bk_pack_reads_flat_ends and the FASTQ readers of
`bronko call` (fastq_pack.hpp, through pack_cat --ends) -- against the Python restatement of the contract (tests/primer_ref.py);
what `bronko call` refuses in a primer file; the new symbols of the C ABI."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, pack_reads, pack_reads_ends

from tests import primer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCAT = os.path.join(ROOT, "bronko_amd", "bin", "pack_cat")
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def pcat():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bronko_amd", "host"), "../bin/pack_cat"])
    return PCAT


@pytest.fixture(scope="module")
def bronko():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bronko_amd", "host"), "../bin/bronko"])
    return BRONKO


def some_reads(n, seed, lengths=(150, 32, 300, 20, 0, 21, 75)):
    """reads with an N at the first letter, at the last letter and in the middle, lower-case reads, reads shorter than k, empty ones"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for i in range(n):
        ln = int(lengths[i % len(lengths)])
        s = bytearray(acgt[rng.integers(0, 4, ln)].tobytes())
        pat = i % 11
        if ln:
            if pat == 1:
                s[0] = ord("N")
            elif pat == 2:
                s[-1] = ord("N")
            elif pat == 3:
                s[ln // 2] = ord("N")
            elif pat == 4:
                s[0] = s[-1] = ord("n")
            elif pat == 5:
                s = bytearray(bytes(s).lower())
            elif pat == 6 and ln > 60:
                s[25] = s[ln - 26] = ord("N")            # three runs: the first and the last touch an end
            elif pat == 7 and ln > 30:
                s[10] = ord("N")                         # the first run is shorter than k: no record, no flag for it
        out.append(bytes(s))
    return out


def unpack(words, lens):
    out = []
    for w, l in zip(words, lens):
        out.append(bytes(b"ACGT"[(int(w[i >> 4]) >> (2 * (i & 15))) & 3] for i in range(int(l))))
    return out


@pytest.mark.parametrize("stride_words", [None, 2, 3])
def test_pack_reads_flat_ends_equals_the_contract(stride_words):
    """Every record's flags, and the records themselves unchanged; a small stride cuts the reads into chunks, which carry no flag."""
    reads = some_reads(600, 3)
    k = 21
    w, l, e = pack_reads_ends(reads, k, stride_words)
    w0, l0 = pack_reads(reads, k, stride_words)
    assert np.array_equal(w, w0) and np.array_equal(l, l0)
    want = primer_ref.end_flags(reads, k, stride_words)
    assert unpack(w, l) == [b for b, _ in want]
    assert e.tolist() == [f for _, f in want]
    assert set(e.tolist()) == ({0, 1, 2, 3} if stride_words is None else {0, 1, 2, 3})
    if stride_words == 2:   # 32-base records: a 150-base read is chunks only
        assert 0 in e.tolist() and sum(f == 3 for f in e.tolist()) > 0   # (the 32-, 21-base reads are whole records)


def test_pack_reads_flat_ends_sizing_call_and_null_flags():
    L = _ffi.load()
    reads = some_reads(50, 4)
    flat = np.frombuffer(b"".join(reads) + b"A", np.uint8)
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    n = L.bk_pack_reads_flat_ends(flat.ctypes.data, off.ctypes.data, len(reads), 21, 10, None, None, None, 0)
    assert n == L.bk_pack_reads_flat(flat.ctypes.data, off.ctypes.data, len(reads), 21, 10, None, None, 0) > 0
    words = np.zeros((n, 10), np.uint32)
    lens = np.zeros(n, np.uint16)
    assert L.bk_pack_reads_flat_ends(flat.ctypes.data, off.ctypes.data, len(reads), 21, 10, words.ctypes.data, lens.ctypes.data, None, n) == n


def fastq(reads, quals=None, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i, r in enumerate(reads):
        q = quals[i] if quals is not None else b"I" * len(r)
        out.append(b"@r%d" % i + nl + r + nl + b"+" + nl + q + nl)
    return b"".join(out)


def quals_for(reads, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        qv = rng.integers(25, 41, len(r))
        qv[rng.random(len(r)) < 0.03] = 5
        if len(r):
            if i % 7 == 1:
                qv[0] = 2            # the first letter masked: no 5' flag
            elif i % 7 == 2:
                qv[-1] = 2           # the last letter masked: no 3' flag
            elif i % 7 == 3:
                qv[:] = 40
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


def pack_cat(pcat, path, k, threads, min_qual=0):
    cmd = [pcat, path, str(k), str(threads), "--ends"] + (["--min-qual=%d" % min_qual] if min_qual else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split(b"\n")
    assert lines[-2].startswith(b"reads ")
    return [(ln.split(b"\t")[0], int(ln.split(b"\t")[1])) for ln in lines[:-2]]


@pytest.mark.parametrize("min_qual", [0, 20])
@pytest.mark.parametrize("gz", [False, True])
def test_fastq_packer_end_flags_equal_the_contract(pcat, tmp_path, min_qual, gz):
    """The line loop (one thread) and the parallel reader (four): a file larger than a piece (4 MB), so that reads span pieces;
    CRLF line ends; with qualities, a masked first or last letter takes the flag away."""
    reads = some_reads(30000, 9, lengths=(150, 151, 33, 300, 20, 0, 21))
    quals = quals_for(reads, 10)
    text = fastq(reads, quals, crlf=True)
    assert len(text) > (5 << 20)
    path = str(tmp_path / ("r.fastq" + (".gz" if gz else "")))
    with (gzip.open(path, "wb", compresslevel=1) if gz else open(path, "wb")) as f:
        f.write(text)
    want = primer_ref.end_flags(reads, 21, quals=quals, min_qual=min_qual)
    assert len({f for _, f in want}) == 4
    for threads in (1, 4):
        assert pack_cat(pcat, path, 21, threads, min_qual) == want, threads


def test_fastq_packer_no_flags_on_the_chunks_of_a_cut_run(pcat, tmp_path):
    """Reads longer than a record (70000 > 65520 bases) are cut into chunks that carry no flag; reads of 40 kb span the pieces."""
    reads = some_reads(40, 5, lengths=(70000, 150, 40000, 66000))
    quals = quals_for(reads, 6)
    path = str(tmp_path / "long.fastq")
    open(path, "wb").write(fastq(reads, quals))
    for min_qual in (0, 20):
        want = primer_ref.end_flags(reads, 21, quals=quals, min_qual=min_qual)
        assert any(f == 0 and len(b) > 60000 for b, f in want)
        for threads in (1, 4):
            assert pack_cat(pcat, path, 21, threads, min_qual) == want, (min_qual, threads)


def test_without_ends_pack_cat_prints_what_it_printed(pcat, tmp_path):
    reads = some_reads(500, 2)
    path = str(tmp_path / "r.fastq")
    open(path, "wb").write(fastq(reads))
    r = subprocess.run([pcat, path, "21", "1"], stdout=subprocess.PIPE, timeout=60)
    assert b"\t" not in r.stdout


# ---- the contract's own reference: the vectorised form the GPU tests use equals the letter-by-letter one --------------------------
def test_reference_trim_lengths_agree():
    from bronko_amd import synth
    g = synth.read_fasta_bytes(os.path.join(GOLDEN, "HPV16.fa"))
    amps = primer_ref.tile_amplicons(g, 1)
    primers = [p for a in amps for p in a[2:]]
    reads = primer_ref.amplicon_reads(g, g, amps, 300, 150, 2) + primer_ref.edge_reads(g, amps, 150)
    for m in (0, 1, 3):
        p5, p3, e0, s1 = primer_ref.trim_lengths_all(reads, primers, m)
        for i, r in enumerate(reads):
            assert (int(p5[i]), int(p3[i])) == primer_ref.trim_lengths(r, primers, m), (m, i, r)
        assert (p5 > 0).sum() > 100 and (p3 > 0).sum() > 10
    assert primer_ref.trim_lengths(b"ACGTACGTACGTAAAAACCCCC", [b"ACGTACGTACGT"], 0) == (12, 0)
    assert primer_ref.trim_lengths(b"ACGTNCGTACGTAAAAACCCCC", [b"ACGTACGTACGT"], 3) == (0, 0)          # interrupted by an N
    assert primer_ref.trim_lengths(b"AACGTACGTACGTAAAACCCCC", [b"ACGTACGTACGT"], 1) == (0, 0)          # not anchored
    assert primer_ref.trim_lengths(b"GGGGGTTTTT" + primer_ref.revcomp(b"ACGTACGTACGA"), [b"ACGTACGTACGA"], 0) == (0, 12)
    assert primer_ref.trim_lengths(b"GGGGGTTTTT" + primer_ref.revcomp(b"ACGTACGTACGA")[:-1], [b"ACGTACGTACGA"], 3) == (0, 0)   # partial


# ---- bronko call --primers: what is refused before any device is touched ---------------------------------------------------------
def call_with(bronko, tmp_path, extra):
    fq = str(tmp_path / "r.fastq")
    open(fq, "wb").write(fastq(some_reads(10, 1)))
    return subprocess.run([bronko, "call", "-d", os.path.join(GOLDEN, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")] + extra,
                          capture_output=True, text=True, timeout=120)


def primer_file(tmp_path, records, name="primers.fa", gz=False):
    path = str(tmp_path / (name + (".gz" if gz else "")))
    text = "".join(">p%d\n%s\n" % (i + 1, s) for i, s in enumerate(records)).encode()
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(text)
    return path


GOOD = "ACGTACGTACGTACGTAC"


@pytest.mark.parametrize("case", ["missing file", "empty file", "symbol", "short", "long", "too many", "mismatches 4", "mismatches -1",
                                  "mismatches without primers", "gzip symbol"])
def test_cli_refuses_bad_primers(bronko, tmp_path, case):
    needle = []
    if case == "missing file":
        extra = ["--primers", str(tmp_path / "nope.fa")]
        needle = ["nope.fa"]
    elif case == "empty file":
        extra = ["--primers", primer_file(tmp_path, [])]
        needle = ["primers.fa", "no records"]
    elif case == "symbol":
        extra = ["--primers", primer_file(tmp_path, [GOOD, GOOD[:9] + "R" + GOOD[10:], GOOD])]
        needle = ["primers.fa", "record 2", "'R'"]
    elif case == "gzip symbol":
        extra = ["--primers", primer_file(tmp_path, [GOOD, GOOD, GOOD[:3] + "N" + GOOD[4:]], gz=True)]
        needle = ["primers.fa.gz", "record 3", "'N'"]
    elif case == "short":
        extra = ["--primers", primer_file(tmp_path, [GOOD, "ACGTACGTACG"])]
        needle = ["primers.fa", "record 2", "11 bases"]
    elif case == "long":
        extra = ["--primers", primer_file(tmp_path, ["ACGT" * 16 + "A", GOOD])]
        needle = ["primers.fa", "record 1", "65 bases"]
    elif case == "too many":
        extra = ["--primers", primer_file(tmp_path, [GOOD] * 1025)]
        needle = ["primers.fa", "1025", "1024"]
    elif case == "mismatches 4":
        extra = ["--primers", primer_file(tmp_path, [GOOD]), "--primer-mismatches", "4"]
        needle = ["between 0 and 3"]
    elif case == "mismatches -1":
        extra = ["--primers", primer_file(tmp_path, [GOOD]), "--primer-mismatches=-1"]
        needle = ["between 0 and 3"]
    else:
        extra = ["--primer-mismatches", "1"]
        needle = ["--primers"]
    res = call_with(bronko, tmp_path, extra)
    assert res.returncode == 1, (res.stdout, res.stderr)
    for s in needle:
        assert s in res.stdout + res.stderr, (s, res.stdout, res.stderr)


def test_cli_usage_names_the_options(bronko):
    res = subprocess.run([bronko, "--help"], capture_output=True, text=True, timeout=60)
    assert "--primers" in res.stdout + res.stderr and "--primer-mismatches" in res.stdout + res.stderr


def test_library_exports_the_primer_symbols():
    hdr = open(os.path.join(ROOT, "include", "bronko_hip.h")).read()
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        for s in ("bk_primers_set", "bk_push_reads_packed_ends", "bk_push_reads_packed_ends_device", "bk_primer_stats", "bk_pack_reads_flat_ends"):
            assert hasattr(L, s) and s in _ffi.SYMBOLS and s + "(" in hdr, s
        assert L.bk_abi_version() == 8
