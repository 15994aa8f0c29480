"""--min-base-qual on the host (no GPU): a base whose quality byte is below '!' + Q (Phred+33) is packed as an N.  The definition the
tests hold the code to: every packed record equals what the same reader makes of the file with those bases replaced by N, for the
line loop (one thread) and the parallel reader (fastq_pack.hpp), plain and gzip, records across pieces; the option's range."""
import gzip
import os
import subprocess

import numpy as np
import pytest

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


def mask_fastq(text, q):
    """the reads' text with every base whose quality byte is below '!' + q replaced by N (the definition of the option)"""
    lines = text.split(b"\n")
    thr = 33 + q
    for i in range(1, len(lines), 4):
        if i + 2 >= len(lines):
            break
        s, ql = lines[i], lines[i + 2]
        cr = s.endswith(b"\r")
        s0, q0 = s.rstrip(b"\r"), ql.rstrip(b"\r")
        assert len(s0) == len(q0)
        a = np.frombuffer(s0, np.uint8).copy()
        a[np.frombuffer(q0, np.uint8) < thr] = ord("N")
        lines[i] = a.tobytes() + (b"\r" if cr else b"")
    return b"\n".join(lines)


def quality_reads(n_reads, seed, lengths=(150,), crlf=False, p_low=0.05):
    """reads with quality lines: mostly high, low bases at random and in the patterns that cut the packer's words and runs"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGTacgt", np.uint8)
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n_reads):
        ln = int(lengths[i % len(lengths)])
        s = acgt[rng.integers(0, 4 if i % 11 else 8, ln)].copy()   # (lower case now and then)
        if i % 13 == 3 and ln:
            s[int(rng.integers(0, ln))] = ord("N")
        qv = rng.integers(25, 42, ln)
        qv[rng.random(ln) < p_low] = rng.integers(0, 19)
        pat = i % 8
        if pat == 1:
            qv[[p for p in (15, 16, 31, 32) if p < ln]] = 0          # word boundaries
        elif pat == 2:
            qv[:] = 0                                                # the whole read masked
        elif pat == 3 and ln > 60:
            qv[:] = 40; qv[20] = qv[41] = 0                          # a run of k - 1 = 20 between two masks (k = 21)
        elif pat == 4 and ln > 60:
            qv[:] = 40; qv[20] = qv[42] = 0                          # a run of exactly k
        elif pat == 5:
            qv[:] = 40                                               # nothing masked
        elif pat == 6 and ln:
            qv[-1] = 0                                               # the last base
        q = (qv + 33).astype(np.uint8).tobytes()
        out.append(b"@q%d\n".replace(b"\n", nl) % i + s.tobytes() + nl + b"+" + nl + q + nl)
    return b"".join(out)


def run(pcat, path, k, threads, min_qual=None, ok=True):
    cmd = [pcat, path, str(k), str(threads)] + ([] if min_qual is None else ["--min-qual=%d" % min_qual])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return r.stdout


def write(path, text, gz=False):
    if gz:
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(text)
    else:
        open(path, "wb").write(text)
    return path


@pytest.mark.parametrize("q", [1, 20, 30])
@pytest.mark.parametrize("lengths", [(32,), (150,), (300, 21, 0, 75), (70000, 150)])
def test_masked_packing_equals_n_substituted_text(pcat, tmp_path, q, lengths):
    """pack_lines with qualities = pack_lines on N-substituted lines: reads of 32, 150, 300 bases, empty and k-long ones, and reads
    longer than a record (70000 > 65535 bases: cut into chunks)."""
    n = 40 if lengths[0] == 70000 else 3000
    t = quality_reads(n, q * 7 + len(lengths), lengths)
    p = write(str(tmp_path / "r.fastq"), t)
    m = write(str(tmp_path / "m.fastq"), mask_fastq(t, q))
    want = run(pcat, m, 21, 1)
    for threads in (1, 4):
        assert run(pcat, p, 21, threads, q) == want, threads
    assert run(pcat, p, 21, 1) != want   # (the masks change something)


def test_min_qual_zero_changes_nothing(pcat, tmp_path):
    t = quality_reads(2000, 5, (150, 90))
    p = write(str(tmp_path / "r.fastq"), t)
    for threads in (1, 3):
        assert run(pcat, p, 21, threads, 0) == run(pcat, p, 21, threads)


@pytest.mark.parametrize("gz", [False, True])
def test_records_across_pieces(pcat, tmp_path, gz):
    """The parallel reader carries the unfinished record from piece to piece: 40 kb reads (a record spans pieces of a 4 MB slice or
    of the inflate's output), and many short reads (a file larger than 4 MB), CRLF line ends; its records equal the line loop's."""
    long_t = quality_reads(300, 1, (40000, 0, 39999), p_low=0.01)
    short_t = quality_reads(40000, 2, (150, 151, 33), crlf=True)
    for name, t in (("long", long_t), ("short", short_t)):
        p = write(str(tmp_path / (name + ".fastq" + (".gz" if gz else ""))), t, gz)
        m = write(str(tmp_path / (name + "_m.fastq")), mask_fastq(t, 20))
        want = run(pcat, m, 31, 1)
        for threads in (1, 2, 8):
            assert run(pcat, p, 31, threads, 20) == want, (name, threads)


def test_a_last_record_without_line_end(pcat, tmp_path):
    t = quality_reads(500, 3, (150,))[:-1]
    p = write(str(tmp_path / "r.fastq"), t)
    m = write(str(tmp_path / "m.fastq"), mask_fastq(t, 25))
    want = run(pcat, m, 21, 1)
    for threads in (1, 4):
        assert run(pcat, p, 21, threads, 25) == want


@pytest.mark.parametrize("cut", ["short quality", "long quality", "no quality line"])
def test_a_quality_line_of_another_length_is_an_error_only_when_masking(pcat, tmp_path, cut):
    t = quality_reads(3000, 4, (150,))
    lines = t.split(b"\n")
    rec = 1234
    if cut == "short quality":
        lines[4 * rec + 3] = lines[4 * rec + 3][:-1]
    elif cut == "long quality":
        lines[4 * rec + 3] += b"I"
    else:
        rec = 2999
        lines = lines[:4 * rec + 2] + [b""]   # (the file ends behind the last record's sequence line)
    p = write(str(tmp_path / "bad.fastq"), b"\n".join(lines))
    for threads in (1, 4):
        run(pcat, p, 21, threads)                          # without masking nothing new is checked
        r = run(pcat, p, 21, threads, 20, ok=False)
        assert r.returncode == 1, (threads, r.stderr)
        err = r.stderr.decode()
        assert "bad.fastq" in err and "record %d" % (rec + 1) in err, err


@pytest.mark.parametrize("value", [["--min-base-qual", "94"], ["--min-base-qual=-1"], ["--min-base-qual", "-5"]])
def test_cli_refuses_a_quality_outside_0_to_93(bronko, tmp_path, value):
    fq = write(str(tmp_path / "r.fastq"), quality_reads(10, 1))
    res = subprocess.run([bronko, "call", "-d", os.path.join(GOLDEN, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")] + value,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1, (res.stdout, res.stderr)
    assert "quality" in (res.stdout + res.stderr).lower()


def test_cli_usage_names_the_option(bronko):
    res = subprocess.run([bronko, "--help"], capture_output=True, text=True, timeout=60)
    assert "--min-base-qual" in res.stdout + res.stderr


@pytest.mark.parametrize("value", ["94", "-1", "x", ""])
def test_pack_cat_refuses_a_quality_outside_0_to_93(pcat, tmp_path, value):
    p = write(str(tmp_path / "r.fastq"), quality_reads(10, 1))
    r = subprocess.run([pcat, p, "21", "1", "--min-qual=" + value], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"0..93" in r.stderr, r.stderr
