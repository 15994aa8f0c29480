"""`bronko call --regions / --region-window` without a GPU: the host twin of region_depth_kernel (caller.cpp region_depths) against
the Python restatement (tests/regions_ref.py) on the crafted regions and a random mix; the BED reader and resolver; the window
tiling; the TSV writer byte for byte; the argument checks of the binary, every one of which exits 1 before a device is touched."""
import gzip
import os
import random
import subprocess

import pytest

from bronko_amd import _ffi, hostlib
from bronko_amd.hostlib import HostIndex
from tests import pileup_cases, regions_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
K = pileup_cases.K


@pytest.fixture(scope="module")
def indexes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = HostIndex.build_mem(K, regions_ref.layout(name).files)
        return made[name]
    yield get
    for ix in made.values():
        ix.close()


def _compare(ix, case, regions, min_depth):
    lay = case.layout
    for f in range(len(lay.file_seqs)):                          # every genome file as the selected one
        want_rows, want_tallies = regions_ref.expected(case, regions, min_depth, file_id=f)
        rows, tallies = hostlib.region_depths(ix, f, case.fwd, case.rev, regions, min_depth)
        assert tallies == want_tallies, (case.name, min_depth, f)
        assert rows == want_rows, (case.name, min_depth, f, [i for i in range(len(rows)) if rows[i] != want_rows[i]][:5])
    return len(regions)


@pytest.mark.parametrize("name", ["lengths", "multi", "long"])
def test_host_twin_on_the_crafted_regions(indexes, name):
    lay = regions_ref.layout(name)
    regions = regions_ref.shape_regions(lay)
    lens = {r[3] - r[2] for r in regions if r[0] == lay.target}
    assert {1, 2, 3, 63, 64, 65, 255, 256, 257} <= lens
    if name == "long":
        assert {regions_ref.LDS - 1, regions_ref.LDS, regions_ref.LDS + 1, 3100} <= lens
    for pattern in regions_ref.PATTERNS:
        case = regions_ref.pattern_case(lay, pattern)
        for d in regions_ref.DEPTHS:
            _compare(indexes(name), case, regions, d)


def test_host_twin_on_a_random_mix(indexes):
    lay = regions_ref.layout("long")
    rng = random.Random(77)
    n = 0
    for draw in range(4):                                        # 4 random pileups x 50 regions of 1..3000 positions
        case = regions_ref.pattern_case(lay, "random", seed=draw)
        regions = regions_ref.random_regions(lay, rng, 50)
        n += _compare(indexes("long"), case, regions, rng.choice([1, 2, 10, 300, 5000]))
    assert n == 200


def test_the_patterns_are_what_they_are_for():
    """Stated on the restatement itself: the lower median, the boundary rank, the outlier, the thresholds."""
    row = regions_ref.region_row
    assert row([4, 9], 1)[3] == 4 and row([9, 4, 7], 1)[3] == 7 and row([5], 1) == (5, 5, 5, 5, 1)
    assert row([5, 500] * 8, 10) == (8 * 505, 5, 500, 5, 8) and row([5, 500] * 8 + [5], 10)[3] == 5 and row([500, 5] * 8 + [500], 10)[3] == 500
    assert row([1, 2, 2 * 10 ** 12, 3], 1)[3] == 2 and row([2 * 10 ** 12] * 3 + [1], 1)[3] == 2 * 10 ** 12
    assert [row([9, 10, 11], d)[4] for d in (9, 10, 11, 12)] == [3, 2, 1, 0]
    lay = regions_ref.layout("lengths")
    case = regions_ref.pattern_case(lay, "outlier")
    rows, _ = regions_ref.expected(case, [(lay.target, len(lay.seqs) - 1, 0, lay.seqs[-1][1], ".")], 10)
    assert 2 * 10 ** 12 <= rows[0][2] < 2 * 10 ** 12 + 10 and rows[0][3] < 10
    fwd_only = regions_ref.pattern_case(lay, "forward_only")
    assert not fwd_only.rev[lay.seqs[0][0] * 4:].any() and fwd_only.fwd.any()
    assert regions_ref.mean_text(0, 7) == "0.00" and regions_ref.mean_text(21, 20) == "1.05" and regions_ref.mean_text(399, 100) == "3.99"
    assert regions_ref.mean_text(2, 3) == "0.66"                 # truncated, not rounded


# ---- the BED reader and the resolver --------------------------------------------------------------------------------------------------
BED = ("# a comment\n"
       "track name=amplicons\n"
       "browser position x:1-2\n"
       "\n"
       "multi_s0\t0\t330\tamp_1\t60\t+\n"
       "multi_s2\t10\t20\n"
       "d1\t5\t130\tdecoy\n"
       "multi_s3\t400\t401\t\n"
       "multi_s0\t0\t330\tamp_1\n")
BED_REGIONS = [(1, 0, 0, 330, "amp_1"), (1, 2, 10, 20, "."), (0, 0, 5, 130, "decoy"), (1, 3, 400, 401, "."), (1, 0, 0, 330, "amp_1")]


def test_bed_plain_gzip_cr_and_skipped_lines(indexes, tmp_path):
    ix = indexes("multi")
    plain, gz, cr = str(tmp_path / "a.bed"), str(tmp_path / "a.bed.gz"), str(tmp_path / "cr.bed")
    open(plain, "w").write(BED)
    with gzip.open(gz, "wb") as f:
        f.write(BED.encode())
    open(cr, "wb").write(BED.replace("\n", "\r\n").encode())
    assert hostlib.bed_regions(ix, plain) == BED_REGIONS
    assert hostlib.bed_regions(ix, gz) == BED_REGIONS
    assert hostlib.bed_regions(ix, cr) == BED_REGIONS
    no_newline = str(tmp_path / "n.bed")
    open(no_newline, "w").write("multi_s1\t0\t57")
    assert hostlib.bed_regions(ix, no_newline) == [(1, 1, 0, 57, ".")]
    empty = str(tmp_path / "e.bed")
    open(empty, "w").write("# nothing\n")
    assert hostlib.bed_regions(ix, empty) == []


def test_bed_name_in_several_files_gives_one_region_per_file(tmp_path):
    rng = random.Random(5)
    files = [("a", [("chr1 first", pileup_cases.random_sequence(rng, 80)), ("chrA", pileup_cases.random_sequence(rng, 40))]),
             ("b", [("chrB", pileup_cases.random_sequence(rng, 50)), ("chr1 second", pileup_cases.random_sequence(rng, 90))])]
    ix = HostIndex.build_mem(K, files)
    try:
        bed = str(tmp_path / "s.bed")
        open(bed, "w").write("chr1\t10\t80\tboth\nchrB\t0\t50\n")
        assert hostlib.bed_regions(ix, bed) == [(0, 0, 10, 80, "both"), (1, 1, 10, 80, "both"), (1, 0, 0, 50, ".")]
        open(bed, "w").write("chr1\t10\t81\tboth\n")             # fits b's chr1 (90), not a's (80)
        with pytest.raises(RuntimeError) as ei:
            hostlib.bed_regions(ix, bed)
        assert "line 1" in str(ei.value) and "s.bed" in str(ei.value)
    finally:
        ix.close()


@pytest.mark.parametrize("text, line, word", [
    ("multi_s0\t0\t10\nmulti_s0\tx\t10\n", 2, "start"),
    ("multi_s0\t-1\t10\n", 1, "start"),
    ("multi_s0\t0\t1e3\n", 1, "end"),
    ("multi_s0\t0\t\n", 1, "end"),
    ("#c\n\nmulti_s0\t10\t10\n", 3, "below"),
    ("multi_s0\t20\t10\n", 1, "below"),
    ("multi_s0\t0\n", 1, "column"),
    ("multi_s0 0 10\n", 1, "column"),
    ("multi_s0\t0\t10\nnobody\t0\t10\n", 2, "nobody"),
    ("multi_s1\t0\t57\nmulti_s1\t0\t58\n", 2, "beyond"),
])
def test_bed_errors_name_the_file_and_the_line(indexes, tmp_path, text, line, word):
    bed = str(tmp_path / "bad.bed")
    open(bed, "w").write(text)
    with pytest.raises(RuntimeError) as ei:
        hostlib.bed_regions(indexes("multi"), bed)
    msg = str(ei.value)
    assert "bad.bed" in msg and "line %d" % line in msg and word in msg, msg


def test_bed_takes_65536_regions_and_no_more(indexes, tmp_path):
    bed = str(tmp_path / "many.bed")
    open(bed, "w").write("multi_s0\t0\t1\n" * 65536)
    assert len(hostlib.bed_regions(indexes("multi"), bed)) == 65536
    open(bed, "a").write("multi_s0\t0\t1\n")
    with pytest.raises(RuntimeError) as ei:
        hostlib.bed_regions(indexes("multi"), bed)
    assert "65536" in str(ei.value)


@pytest.mark.parametrize("window", [1, 7, 64, 330, 5000])
def test_window_tiling(indexes, window):
    lay = regions_ref.layout("multi")
    lens = [[n for _, n in seqs] for seqs in lay.file_seqs]
    got = hostlib.window_regions(indexes("multi"), window)
    assert got == regions_ref.window_regions(lens, window)
    assert sum(r[3] - r[2] for r in got) == lay.total_cells


def test_window_count_above_the_limit_says_to_raise_it():
    """1025 files x 256 sequences x 16 positions (shorter than k: no k-mers) are 4100 windows of 1 more than 2^22."""
    files = [("f%d" % f, [("s%d_%d" % (f, j), b"ACGTACGTACGTACGT") for j in range(256)]) for f in range(1025)]
    ix = HostIndex.build_mem(K, files)
    try:
        with pytest.raises(RuntimeError) as ei:
            hostlib.window_regions(ix, 1)
        assert "raise" in str(ei.value) and str((1 << 22) + 4096) in str(ei.value)
        assert len(hostlib.window_regions(ix, 16)) == 1025 * 256
        with pytest.raises(RuntimeError):
            hostlib.window_regions(ix, 0)
    finally:
        ix.close()


# ---- the writer ------------------------------------------------------------------------------------------------------------------------
def test_writer_byte_for_byte(indexes, tmp_path):
    ix, lay = indexes("multi"), regions_ref.layout("multi")
    regions = [(1, 0, 0, 330, "amp_1"), (0, 0, 0, 130, "decoy"), (1, 1, 0, 20, "."), (1, 3, 1, 401, "amp 3"), (1, 0, 7, 107, "x"), (1, 2, 0, 3, ".")]
    big = (1 << 53) + 12345
    rows = [(0, 0, 0, 0, 0), (21, 1, 2, 1, 20), (399 * 4, 0, 1000, 3, 57), (big, 1, big, 7, 99), ((1 << 64) - 1, 5, 1 << 63, 6, 3)]
    path = str(tmp_path / "s.regions.tsv")
    hostlib.write_regions_tsv(path, ix, 1, regions, rows, 10)
    got = open(path, "rb").read()
    chroms = [name.split()[0] for name, _ in lay.files[1][1]]
    assert got == regions_ref.tsv_text(10, chroms, regions, 1, rows)
    lines = got.decode().split("\n")
    assert lines[0] == "##min_depth=10" and lines[1] == "chrom\tstart\tend\tname\tlength\tmean\tmin\tmedian\tmax\tcovered" and lines[-1] == ""
    assert lines[2] == "multi_s0\t0\t330\tamp_1\t330\t0.00\t0\t0\t0\t0"
    assert lines[3] == "multi_s1\t0\t20\t.\t20\t1.05\t1\t1\t2\t20"
    assert lines[4] == "multi_s3\t1\t401\tamp 3\t400\t3.99\t0\t3\t1000\t57"
    assert lines[5] == "multi_s0\t7\t107\tx\t100\t%d.%02d\t1\t7\t%d\t99" % (big // 100, big % 100, big)
    assert lines[6] == "multi_s2\t0\t3\t.\t3\t%d.%02d\t5\t6\t%d\t3" % (((1 << 64) - 1) * 100 // 3 // 100, ((1 << 64) - 1) * 100 // 3 % 100, 1 << 63)
    # a genome without a region, and no genome: the two header lines
    hostlib.write_regions_tsv(path, ix, 0, [r for r in regions if r[0] == 1], [], 300)
    assert open(path, "rb").read() == b"##min_depth=300\n" + regions_ref.HEADER.encode()
    hostlib.write_regions_tsv(path, ix, -1, regions, [], 1)
    assert open(path, "rb").read() == b"##min_depth=1\n" + regions_ref.HEADER.encode()
    with pytest.raises(RuntimeError):                            # rows that are not the genome's regions
        hostlib.write_regions_tsv(path, ix, 1, regions, rows[:4], 10)


# ---- the binary's argument checks ----------------------------------------------------------------------------------------------------
def _hpv_chrom(golden_dir):
    ix = HostIndex.load(os.path.join(golden_dir, "hpv.bkdb"))
    try:
        name, seq = ix.files()[0][1][0]
        return name.split()[0], len(seq)
    finally:
        ix.close()


def test_cli_refuses_bad_region_arguments(golden_dir, tmp_path):
    db = os.path.join(golden_dir, "hpv.bkdb")
    chrom, n = _hpv_chrom(golden_dir)
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")

    def bed(name, text):
        p = str(tmp_path / name)
        open(p, "w").write(text)
        return p

    good = bed("good.bed", "%s\t0\t100\tamp\n" % chrom)
    cases = [
        (["--regions", bed("start.bed", "%s\tzero\t100\n" % chrom)], ["start.bed", "line 1", "start"]),
        (["--regions", bed("end.bed", "%s\t0\t100\n%s\t0\t1.5\n" % (chrom, chrom))], ["end.bed", "line 2", "end"]),
        (["--regions", bed("order.bed", "%s\t100\t100\n" % chrom)], ["order.bed", "line 1", "below"]),
        (["--regions", bed("order2.bed", "%s\t101\t100\n" % chrom)], ["order2.bed", "line 1", "below"]),
        (["--regions", bed("cols.bed", "%s\t100\n" % chrom)], ["cols.bed", "line 1", "column"]),
        (["--regions", good, "--region-window", "100"], ["--regions", "--region-window"]),
        (["--region-min-depth", "5"], ["--region-min-depth", "--regions"]),
        (["--regions", good, "--region-min-depth", "0"], ["depth", "at least 1"]),
        (["--region-window", "100", "--region-min-depth", "0"], ["depth", "at least 1"]),
        (["--region-window", "0"], ["window", "at least 1"]),
        (["--regions", bed("chrom.bed", "%s\t0\t100\nchrUnknown\t0\t100\n" % chrom)], ["chrom.bed", "line 2", "chrUnknown"]),
        (["--regions", bed("beyond.bed", "%s\t0\t%d\n%s\t0\t%d\n" % (chrom, n, chrom, n + 1))], ["beyond.bed", "line 2", "beyond"]),
        (["--regions", bed("many.bed", ("%s\t0\t100\n" % chrom) * 65537)], ["many.bed", "65536"]),
        (["--regions", str(tmp_path / "missing.bed")], ["missing.bed"]),
    ]
    for extra, words in cases:
        r = subprocess.run([BRONKO, "call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout, (extra, r.stdout, r.stderr)
        for w in words:
            assert w in r.stdout, (extra, w, r.stdout)
        assert "no HIP device" not in r.stdout                   # refused before any device is touched
    usage = subprocess.run([BRONKO, "--help"], capture_output=True, text=True).stderr
    for opt in ("--regions", "--region-window", "--region-min-depth"):
        assert opt in usage


def test_abi_names_the_region_functions():
    for s in ("bk_regions_set", "bk_sample_region_depths", "bk_sample_download_region_depths"):
        assert s in _ffi.SYMBOLS and hasattr(_ffi.load(), s)
    import ctypes as C
    assert C.sizeof(_ffi.Region) == 16 and C.sizeof(_ffi.RegionDepth) == 40 and C.sizeof(_ffi.RegionSummary) == 32
    assert _ffi.RegionSummary.full.offset == 8
