"""bk_sample_region_depths (region_depth_kernel) against the Python restatement (tests/regions_ref.py): on crafted pileups the way
tests/test_gpu_consensus.py gets them onto the device -- a sample of selection reads is finalized, the device pileup is overwritten,
bk_sample_call selects the genome, then the regions are reported from what is there --, the table's life and the call order of the
C ABI, and `bronko call --regions / --region-window` end to end on reads with a stretch nothing covers.  Every number and every
tally must equal the restatement's: the rule is integer arithmetic, no case is left out for being near anything."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, synth
from tests import helpers, pileup_cases, regions_ref

pytestmark = pytest.mark.gpu
K = pileup_cases.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _to_call(eng, case, reads=True):
    """The case's pileup on the device and bk_sample_call run on it (reads=False: a sample without reads, which selects nothing)."""
    import torch
    from bronko_amd import pack_reads
    from bronko_amd.dist import DeviceVector
    eng.sample_begin()
    if reads:
        words, lens = pack_reads(case.layout.selection_reads(), K)
        eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_download(1, arrays=False)                         # (synchronises: the finalize has written its pileup)
    cells4 = eng.total_cells * 4
    assert cells4 == len(case.fwd)
    dev = torch.as_tensor(DeviceVector(eng.pileup_ptr(), 4 * cells4), device="cuda:0")
    dev.copy_(torch.from_numpy(np.concatenate(case.arrays()).view(np.int64)))
    torch.cuda.synchronize()
    eng.sample_call(1, case.params.apply(eng.call_params()))


def _report(eng, case, regions, depths=regions_ref.DEPTHS, file_id=None):
    """The device's rows and tallies of the regions set on the engine at every D against the restatement; returns the rows compared."""
    n = 0
    fid = case.layout.target if file_id is None else file_id
    for d in depths:
        want_rows, (full, partial, empty) = regions_ref.expected(case, regions, d, file_id=fid)
        eng.sample_region_depths(d)
        summ, rows = eng.download_region_depths()
        assert summ.file_id == fid and summ.n_regions == len(want_rows), (case.name, d)
        assert (summ.full, summ.partial, summ.empty) == (full, partial, empty), (case.name, d)
        if rows != want_rows:
            bad = [i for i in range(len(want_rows)) if rows[i] != want_rows[i]]
            mine = [r for r in regions if r[0] == fid]
            raise AssertionError("%s at D = %d: %d rows differ, first region %r: %r, expected %r" %
                                 (case.name, d, len(bad), mine[bad[0]], rows[bad[0]], want_rows[bad[0]]))
        n += len(rows)
    return n


@pytest.fixture(scope="module")
def engines(oracle):
    """An engine per layout, made inside the first test that wants it."""
    made = {}

    def get(name):
        if name not in made:
            ix = oracle.Index.build_mem(K, regions_ref.layout(name).files)
            made[name] = (ix, helpers.engine_from_oracle_index(ix))
        return made[name][1]
    yield get
    for ix, eng in made.values():
        eng.close()
        ix.close()


@pytest.mark.parametrize("name", ["lengths", "multi", "long"])
def test_crafted_regions_and_patterns(engines, name):
    lay = regions_ref.layout(name)
    regions = regions_ref.shape_regions(lay)
    lens = {r[3] - r[2] for r in regions if r[0] == lay.target}
    assert {1, 2, 3, 63, 64, 65, 255, 256, 257} <= lens and any(r[0] != lay.target for r in regions)
    if name == "long":                                           # around the LDS buffer, and a whole sequence longer than it
        assert {regions_ref.LDS - 1, regions_ref.LDS, regions_ref.LDS + 1, 3100} <= lens
    eng = engines(name)
    eng.regions_set(regions)
    n = 0
    for pattern in regions_ref.PATTERNS:
        case = regions_ref.pattern_case(lay, pattern)
        _to_call(eng, case)
        n += _report(eng, case, regions)
    assert n == len(regions_ref.PATTERNS) * 3 * sum(1 for r in regions if r[0] == lay.target)
    eng.regions_set([])


def test_more_regions_than_one_wave_of_workgroups(engines):
    """A window of one position over every genome: 4052 workgroups of the target's slice (a device holds 2048 of them at once), and
    the same positions as windows of 3 and of 64."""
    lay = regions_ref.layout("lengths")
    eng = engines("lengths")
    lens = [[n for _, n in seqs] for seqs in lay.file_seqs]
    case = regions_ref.pattern_case(lay, "random", seed=9)
    for window in (1, 3, 64):
        regions = regions_ref.window_regions(lens, window)
        eng.regions_set(regions)
        _to_call(eng, case)
        n = _report(eng, case, regions, depths=[10])
        assert n == sum((ln + window - 1) // window for ln in lens[lay.target])
        if window == 1:
            assert n == 4052 > 2048
    eng.regions_set([])


def test_random_mix(engines):
    import random
    lay = regions_ref.layout("long")
    eng = engines("long")
    rng = random.Random(78)
    for draw in range(4):
        case = regions_ref.pattern_case(lay, "random", seed=draw)
        regions = regions_ref.random_regions(lay, rng, 50)
        eng.regions_set(regions)
        _to_call(eng, case)
        _report(eng, case, regions, depths=[rng.choice([1, 2, 10, 300, 5000])])
    eng.regions_set([])


def test_two_samples_in_a_row_and_on_a_fork(oracle):
    """A pileup that covers the long genome, then one of the short genome of the same files, then a sparse one of the long genome
    again, on one engine -- rows and tallies of the sample before must not show --, the same on a fork of that engine, which sets its
    own table, and once more on the engine itself; then the table replaced and cleared between samples."""
    lay = regions_ref.layout("lengths")
    heavy = regions_ref.pattern_case(lay, "rising")
    sparse = regions_ref.pattern_case(lay, "zero")
    for cell0, n in lay.seqs:
        for i in range(cell0 % 7, n, 37):
            sparse.fwd[(cell0 + i) * 4 + 2] = np.uint64(4000)
    short_lay = pileup_cases.Layout("lengths_decoy", lay.files, 0)            # the other genome of the same files
    short = regions_ref.pattern_case(short_lay, "thresholds")
    assert sum(n for _, n in short_lay.seqs) == 150 < sum(n for _, n in lay.seqs)
    regions = regions_ref.shape_regions(lay)
    assert 0 < sum(1 for r in regions if r[0] == 0) < sum(1 for r in regions if r[0] == 1)
    ix = oracle.Index.build_mem(K, lay.files)
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    try:
        eng.regions_set(regions)
        with pytest.raises(BronkoError) as ei:                   # a fork has no table of its parent's
            _to_call(fork, heavy)
            fork.sample_region_depths(10)
        assert ei.value.status == -5
        fork.regions_set(regions)
        for e in (eng, fork, eng):
            for case in (heavy, short, sparse):
                _to_call(e, case)
                _report(e, case, regions)
        # replaced between samples: fewer regions, other ranges; then more again; then cleared
        few = [(1, 18, 5, 900, "a"), (0, 0, 0, 150, "decoy"), (1, 0, 0, 1, "b")]
        eng.regions_set(few)
        _to_call(eng, heavy)
        assert _report(eng, heavy, few) == 3 * 2
        _to_call(eng, short)
        assert _report(eng, short, few) == 3 * 1
        eng.regions_set(regions)
        _to_call(eng, sparse)
        _report(eng, sparse, regions)
        eng.regions_set([])
        _to_call(eng, heavy)
        with pytest.raises(BronkoError) as ei:
            eng.sample_region_depths(10)
        assert ei.value.status == -5 and "regions" in str(ei.value)
        _to_call(fork, heavy)                                    # the fork's table is its own
        _report(fork, heavy, regions, depths=[10])
    finally:
        fork.close()
        eng.close()
        ix.close()


def test_selected_genome_without_regions_and_no_genome_selected(engines):
    lay = regions_ref.layout("multi")
    eng = engines("multi")
    case = regions_ref.pattern_case(lay, "equal")
    decoy_only = [(0, 0, 0, 130, "d"), (0, 0, 3, 4, ".")]
    eng.regions_set(decoy_only)
    _to_call(eng, case)                                          # the target is selected, the decoy has the regions
    eng.sample_region_depths(10)
    summ, rows = eng.download_region_depths()
    assert (summ.file_id, summ.n_regions, summ.full, summ.partial, summ.empty) == (lay.target, 0, 0, 0, 0) and rows == []
    eng.regions_set(regions_ref.shape_regions(lay))
    _to_call(eng, case, reads=False)                             # a sample without reads selects nothing
    eng.sample_region_depths(10)
    summ, rows = eng.download_region_depths()
    assert (summ.file_id, summ.n_regions, summ.full, summ.partial, summ.empty) == (-1, 0, 0, 0, 0) and rows == []
    raw = np.full((4, 5), 0xff, np.uint64)                       # ... and nothing is written
    rs = _ffi.RegionSummary()
    assert eng._L.bk_sample_download_region_depths(eng.h, C.byref(rs), raw.ctypes.data_as(C.c_void_p), 4) == 0
    assert rs.file_id == -1 and (raw == 0xff).all()
    eng.regions_set([])


def test_call_order_parameters_and_cap(oracle):
    lay = regions_ref.layout("multi")
    case = regions_ref.pattern_case(lay, "thresholds")
    regions = regions_ref.shape_regions(lay)
    ix = oracle.Index.build_mem(K, lay.files)
    eng = helpers.engine_from_oracle_index(ix)

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        from bronko_amd import pack_reads
        # what bk_regions_set refuses, with the entry named
        for bad, word in (([(2, 0, 0, 1)], "genome file 2"), ([(-1, 0, 0, 1)], "genome file -1"), ([(1, 4, 0, 1)], "sequence 4"),
                          ([(1, 1, 0, 58)], "[0, 58)"), ([(1, 1, 5, 5)], "[5, 5)"), ([(1, 1, 6, 5)], "[6, 5)"), ([(0, 0, 0, 131)], "[0, 131)")):
            st, msg = status(eng.regions_set, [(1, 0, 0, 1)] + bad)
            assert st == -1 and "region 1" in msg and word in msg, msg
        assert eng._L.bk_regions_set(eng.h, None, 5) == -1       # a count without an array
        assert eng._L.bk_regions_set(eng.h, (_ffi.Region * 1)(), (1 << 22) + 1) == -1 and "4194304" in eng._L.bk_last_error().decode()
        assert status(eng.sample_region_depths)[0] == -5         # BK_ERR_STATE: no regions, nothing was ever called
        eng.regions_set(regions)
        assert status(eng.sample_region_depths)[0] == -5         # regions, but nothing was ever called
        eng.sample_begin()
        assert status(eng.sample_region_depths)[0] == -5         # inside a sample
        st, msg = status(eng.regions_set, regions)
        assert st == -5 and "between samples" in msg             # ... where the table cannot be replaced
        assert status(eng.regions_set, [])[0] == -5
        words, lens = pack_reads(lay.selection_reads(), K)
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        assert status(eng.sample_region_depths)[0] == -5         # finalized, but not called
        assert status(eng.download_region_depths)[0] == -5
        _to_call(eng, case)
        st, msg = status(eng.sample_region_depths, 0)
        assert st == -1 and "min_depth" in msg                  # BK_ERR_INVALID, the parameter named
        assert status(eng.download_region_depths)[0] == -5       # called, but no report was made
        eng.sample_region_depths(10)
        want_rows, tallies = regions_ref.expected(case, regions, 10)
        assert len(want_rows) > 7
        summ, rows = eng.download_region_depths(cap=7)           # fewer than there are: `cap` rows, the full count
        assert summ.n_regions == len(want_rows) and rows == want_rows[:7] and (summ.full, summ.partial, summ.empty) == tallies
        raw, rs = np.full((12, 5), 0xff, np.uint64), _ffi.RegionSummary()   # ... and nothing behind them is written
        assert eng._L.bk_sample_download_region_depths(eng.h, C.byref(rs), raw.ctypes.data_as(C.c_void_p), 7) == 0
        assert [tuple(int(v) for v in r) for r in raw[:7]] == want_rows[:7] and (raw[7:] == 0xff).all() and rs.n_regions == len(want_rows)
        assert eng._L.bk_sample_download_region_depths(eng.h, C.byref(rs), None, 100) == 0 and rs.n_regions == len(want_rows)   # out may be NULL
        assert eng._L.bk_sample_download_region_depths(eng.h, None, None, 0) == -1
        summ, rows = eng.download_region_depths(cap=len(want_rows) + 50)
        assert rows == want_rows
        eng.sample_region_depths(300)                            # again with another D on the same sample
        assert eng.download_region_depths()[1] == regions_ref.expected(case, regions, 300)[0]
        eng.regions_set(regions[:5])                             # a new table: the report of the old one is gone
        assert status(eng.download_region_depths)[0] == -5
        eng.sample_region_depths(10)
        assert eng.download_region_depths()[1] == regions_ref.expected(case, regions[:5], 10)[0]
        eng.sample_begin()                                       # the next sample: the selection is no longer this sample's
        assert status(eng.sample_region_depths)[0] == -5
        assert status(eng.download_region_depths)[0] == -5
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        assert status(eng.sample_region_depths)[0] == -5         # ... not before its own bk_sample_call
        eng.sample_call(1)
        eng.sample_region_depths()
        assert eng.download_region_depths()[0].file_id == lay.target
    finally:
        eng.close()
        ix.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
GAP = (3000, 3600)                                               # no read covers these positions of HPV16


def _sample(golden_dir, paired):
    g = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    gm, isnv = synth.sample_genome(g, 31, n_snp=8, n_isnv=4)
    mates = [[], []]
    for part, (lo, hi) in enumerate(((0, GAP[0]), (GAP[1], len(g)))):   # reads of either side of the gap: none reaches into it
        piece = gm[lo:hi]
        shifted = [(p - lo, alt, af) for p, alt, af in isnv if lo <= p < hi]
        n = 4000 * (hi - lo) // len(g)
        if paired:
            c1, c2 = synth.paired_codes(piece, n // 2, 150, 310 + part, isnv=shifted)
            mates[0] += synth.codes_to_ascii(c1)
            mates[1] += synth.codes_to_ascii(c2)
        else:
            mates[0] += synth.codes_to_ascii(synth.single_end_codes(piece, n, 150, 310 + part, isnv=shifted))
    return g, mates[:2 if paired else 1]


@pytest.mark.parametrize("inflate", ["one", "many"])
@pytest.mark.parametrize("paired", [False, True])
def test_cli_regions_end_to_end(oracle, golden_dir, tmp_path, paired, inflate):
    g, mates = _sample(golden_dir, paired)
    paths = []
    for m, reads in enumerate(mates):
        p = str(tmp_path / ("reg_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(reads):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(golden_dir, "hpv.bkdb")
    ix = oracle.Index.load(db)
    try:
        pile = oracle.sample_pileup(ix, mates)
        assert oracle.pick_best_genome(ix, pile.stats.sum(axis=0), pile.present.max(axis=0)) == 0
        files = ix.files()
    finally:
        ix.close()
    chroms = [name.split()[0] for name, _ in files[0][1]]
    assert len(files[0][1][0][1]) == len(g)
    # an amplicon scheme: 400 positions every 350, two of them inside the gap, the last one to the genome's end; plain or gzip
    bed_regions, lines = [], ["# amplicons\n", "track name=scheme\n"]
    for j, s in enumerate(range(0, len(g), 350)):
        e = min(s + 400, len(g))
        name = "amp_%d" % (j + 1) if j % 5 else "."
        bed_regions.append((0, 0, s, e, name))
        lines.append("%s\t%d\t%d%s\n" % (chroms[0], s, e, "" if name == "." else "\t%s\t60\t+" % name))
    bed = str(tmp_path / ("scheme.bed.gz" if paired else "scheme.bed"))
    with (gzip.open if paired else open)(bed, "wb") as f:
        f.write("".join(lines).encode())
    file_seqs, at = [], 0
    for _, seqs in files:
        cur = []
        for _, s in seqs:
            cur.append((at, len(s)))
            at += len(s)
        file_seqs.append(cur)
    depths = regions_ref.cell_depths(pile.fwd_depth, pile.rev_depth)
    windows = regions_ref.window_regions([[n for _, n in seqs] for seqs in file_seqs], 100)

    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    env = dict(os.environ, BRONKO_INFLATE_THREADS="1") if inflate == "one" else dict(os.environ)
    outs = {}
    for name, extra in (("regions", ["--regions", bed]), ("window", ["--region-window", "100", "--region-min-depth", "25"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "--consensus", "-o", out, "-t", "8"] + extra,
                             capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("inflated on" in res.stdout + res.stderr) == (inflate == "many")
        assert ("regions at minimum depth" in res.stdout) == (name != "without")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
        outs[name]["log"] = res.stdout
    stem = "reg_R1"
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", stem + ".consensus.fa", "bronko_overview.tsv", "log"}
    for name in ("regions", "window"):
        assert set(outs[name]) == set(outs["without"]) | {stem + ".regions.tsv"}
        for f in outs["without"]:                                # the VCF, the pileup TSV, the overview and the consensus do not know of the flags
            assert f == "log" or outs[name][f] == outs["without"][f], (name, f)
    for name, regions, d in (("regions", bed_regions, 10), ("window", windows, 25)):
        rows, (full, partial, empty) = regions_ref.report(file_seqs, depths, regions, 0, d)
        assert outs[name][stem + ".regions.tsv"] == regions_ref.tsv_text(d, chroms, regions, 0, rows), name
        assert full >= 1 and empty >= 1, (name, full, partial, empty)   # amplicons and windows inside the gap, and well-covered ones
        assert "Depth of %d regions at minimum depth %d: %d full, %d partial, %d empty" % (len(rows), d, full, partial, empty) in outs[name]["log"]
    gap_rows = [ln.split("\t") for ln in outs["window"][stem + ".regions.tsv"].decode().split("\n")[2:-1] if GAP[0] + 100 <= int(ln.split("\t")[1]) < GAP[1] - 100]
    assert len(gap_rows) == 4 and all(r[9] == "0" for r in gap_rows)
