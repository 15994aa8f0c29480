"""Count-level sweeps on the GPU (tests/level_sweep.py): every read set below runs once per count value that occurs in it, a fork
of the path's engine with ci = cx = c each time, and every level equals the oracle's -- all four arrays, stats, present and the
k-mer total.  What the plain parity tests cannot see (a k-mer counted one off below another k-mer's maximum) moves a k-mer
from one level to another here.  HPV16 (7.9 kb) throughout.

Set G: chunk and read geometry -- read lengths around the scan's 32-base words, 160-base chunks and their 32-base carry, one
substitution at every read offset near the ends and the boundaries, two substitutions straddling the boundaries (Level 2).
Set T: tiles and the deal -- 32-base reads by the tile (64), the chunk (1024), beyond a workgroup's first chunks, over several
pushes, launches and samples.

Cost: a test is one fork, one sample and one download per level (6 to 22 levels per read set, 0.1 to 0.4 M bases per sample) and
the oracle's levels of its read sets, computed once per module by the first test that needs them.  Wall time of each test on an
MI355X (pytest --durations=0; the whole module, 34 cases: 7.0 s, of which 1.6 s build the read sets and the module's engine):

    test_set_g_whole_on_the_release_library                             0.20 / 0.11 / 0.16 / 0.09 s (parts 0 .. 3)
    test_set_g_third_on_the_other_scan_and_finalize_paths               0.15 .. 0.21 s each of 6 (BK_LDS_BINS=512 the longest)
    test_set_g_third_on_three_overlapping_genomes                       0.31 s every genome, 0.21 s selected genome
    test_set_g_third_on_three_overlapping_genomes_with_touch_lists      0.19 .. 0.21 s each of 4
    test_set_g_third_at_the_smallest_and_the_largest_k                  0.25 s (k = 15), 0.57 s (k = 31)
    test_two_mate_files_of_different_read_sets                          0.22 s
    test_set_t_by_the_tile_and_the_chunk                                0.01 .. 0.02 s each of 7
    test_set_t_chunks_beyond_a_workgroups_first                         0.07 .. 0.09 s each of 4
    test_set_t_over_pushes_and_samples                                  0.01 s two pushes, 0.02 s three samples
    test_set_t_over_launches_of_either_parity                           0.09 s two workgroups, 0.06 s three launches a push

Under BK_SPARSE_FINALIZE=1 the three-slice index does take the gathered votes (the testing build reports answers and cells for
all k-mers, no merged bucket, 202336 window BucketInfos for 12646 occurrences x 16).
"""
import os

import pytest

from bronko_amd import synth
from tests import helpers, level_sweep

pytestmark = pytest.mark.gpu

G_PATHS = [{"BK_NO_FUSE": "1"}, {"BK_NO_ITEMS": "1"}, {"BK_REF_IN_LDS": "0"}, {"BK_LDS_BINS": "512"}, {"BK_SPARSE_FINALIZE": "1"},
           {"BK_MAX_LAUNCH_RECORDS": "333"}]
T_RELEASE = (1, 63, 64, 65, 1023, 1024, 1025)
T_TWO_WORKGROUPS = (2047, 2048, 2049, 4097)


def genome():
    return synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))


def three_files(g):
    """Three overlapping slices of HPV16, a dozen substitutions in each: cells of one genome whose k-mers are another's too, or
    are one substitution away from another's (dirty cells)."""
    out = []
    for f, (lo, hi) in enumerate(((0, 4200), (1800, 6100), (3700, len(g)))):
        s = g[lo:hi]
        out.append(("slice%d" % f, [("hpv%d" % f, level_sweep.substitute(s, *range(150 + 97 * f, len(s) - 150, (len(s) - 300) // 12 + 1)))]))
    return out


def g_third_names(k):
    """(at k = 21 the lengths of the third are part 0 of the whole set: one read set, one name, one set of oracle levels)"""
    return ["G part 0" if k == 21 else "G third, k = %d, lengths" % k, "G third, k = %d, pairs" % k]


def g_third(g, k):
    """The third of set G that every path runs, as its two read sets: every third length, every third placement of the pairs."""
    return list(zip(g_third_names(k), (k, k), ([level_sweep.set_g(g, k, level_sweep.G_LENGTHS[0::3])], [level_sweep.set_g_pairs(g, k, every=3)])))


def g_paired(g):
    return ("G paired", 21, [level_sweep.set_g(g, 21, level_sweep.G_LENGTHS[2::3]), level_sweep.set_g_pairs(g, 21)])


def read_sets(g):
    """(name, k, mates) of every read set of this module (tests/test_level_sweep_cpu.py checks them against the sweep's condition)."""
    for j, reads in enumerate(level_sweep.set_g_parts(g, 21)):
        yield "G part %d" % j, 21, [reads]
    for k in (21, 15, 31):
        yield from (s for s in g_third(g, k) if s[0] != "G part 0")
    yield g_paired(g)
    for n in T_RELEASE + T_TWO_WORKGROUPS:
        yield "T %d" % n, 21, [level_sweep.set_t(g, n)]


@pytest.fixture(scope="module")
def sets():
    g = genome()
    return {name: (k, mates) for name, k, mates in read_sets(g)}


@pytest.fixture(scope="module")
def hpv(oracle, golden_dir):
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    yield ix, eng
    eng.close()
    ix.close()


@pytest.fixture(scope="module")
def slices(oracle):
    ix = oracle.Index.build_mem(21, three_files(genome()))
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def expected(oracle, sets):
    """The oracle's levels of a read set on an index: computed once, shared by every path that runs the set."""
    cache = {}

    def get(ix, name):
        key = (ix.k, tuple((fn, tuple(seqs)) for fn, seqs in ix.files()), name)      # the index by its content: k, names and sequences
        if key not in cache:
            k, mates = sets[name]
            cache[key] = level_sweep.oracle_levels(oracle, ix, mates, k)
        return cache[key]
    return get


def _sweep(oracle, expected, sets, ix, eng, name, **kw):
    k, mates = sets[name]
    return level_sweep.level_sweep(oracle, ix, eng, mates, k, expected=expected(ix, name), **kw)


def _engine_with(monkeypatch, ix, env):
    """An engine of the testing library (the testing_lib fixture is on) created under the switches `env`; a switch the library
    does not know would leave the default path to pass in its place."""
    from bronko_amd import _ffi
    library = open(_ffi.TESTING_LIB_PATH, "rb").read()      # a spelling check only: the name exists; that its path ran is not shown
    for name, value in env.items():
        assert name.encode() in library, "%s is no switch of the testing library" % name
        monkeypatch.setenv(name, value)
    return helpers.engine_from_oracle_index(ix)


# ---- set G ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_set_g_whole_on_the_release_library(oracle, hpv, sets, expected, part):
    """The binned scan with its V items fused into the regional finalize: set G whole, by every third length and the pairs."""
    ix, eng = hpv
    levels = _sweep(oracle, expected, sets, ix, eng, "G part %d" % part)
    assert len(levels) >= 8


@pytest.mark.parametrize("env", G_PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_set_g_third_on_the_other_scan_and_finalize_paths(oracle, hpv, sets, expected, monkeypatch, testing_lib, env):
    """Without the fusion (bin_count_kernel sends every V item to the plane), without items (scan_count_kernel and the fold), the
    reference read from global memory, a window of 512 cells (the rest through Level 2), touch lists instead of plane scans, and
    launches of 333 records."""
    ix, _ = hpv
    eng = _engine_with(monkeypatch, ix, env)
    try:
        for name in g_third_names(21):
            _sweep(oracle, expected, sets, ix, eng, name)
    finally:
        eng.close()


@pytest.mark.parametrize("selected_only", [False, True], ids=["every genome", "selected genome"])
def test_set_g_third_on_three_overlapping_genomes(oracle, slices, sets, expected, selected_only):
    """Three files on the release library: dirty cells and dirty_ans, K2a / K2e / K2b; also with the votes of the selected genome
    only (two finalize passes)."""
    eng = helpers.engine_from_oracle_index(slices)
    try:
        for name in g_third_names(21):
            _sweep(oracle, expected, sets, slices, eng, name, pileup_selected_only=selected_only)
    finally:
        eng.close()


@pytest.mark.parametrize("selected_only", [False, True], ids=["every genome", "selected genome"])
@pytest.mark.parametrize("env", [{"BK_SPARSE_FINALIZE": "1"}, {"BK_SPARSE_FINALIZE": "1", "BK_NO_GATHER": "1"}], ids=["gathered votes", "without the gather"])
def test_set_g_third_on_three_overlapping_genomes_with_touch_lists(oracle, slices, sets, expected, monkeypatch, testing_lib, env, selected_only):
    """... with touch lists instead of plane scans: the gathered votes, and the same without the gather."""
    eng = _engine_with(monkeypatch, slices, env)
    try:
        for name in g_third_names(21):
            _sweep(oracle, expected, sets, slices, eng, name, pileup_selected_only=selected_only)
    finally:
        eng.close()


@pytest.mark.parametrize("k", [15, 31])
def test_set_g_third_at_the_smallest_and_the_largest_k(oracle, golden_dir, sets, expected, k):
    ix = oracle.Index.build(k, [os.path.join(golden_dir, "HPV16.fa")])
    eng = helpers.engine_from_oracle_index(ix)
    try:
        for name in g_third_names(k):
            _sweep(oracle, expected, sets, ix, eng, name)
    finally:
        eng.close()
        ix.close()


def test_two_mate_files_of_different_read_sets(oracle, hpv, sets, expected):
    """Paired: the levels are taken over both count tables, every mate file is thresholded on its own."""
    ix, eng = hpv
    _sweep(oracle, expected, sets, ix, eng, "G paired")


# ---- set T ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T_RELEASE)
def test_set_t_by_the_tile_and_the_chunk(oracle, hpv, sets, expected, n):
    """One push of n reads: less than a tile, a tile, a chunk of sixteen, one read more than each."""
    ix, eng = hpv
    _sweep(oracle, expected, sets, ix, eng, "T %d" % n)


@pytest.mark.parametrize("n", T_TWO_WORKGROUPS)
def test_set_t_chunks_beyond_a_workgroups_first(oracle, hpv, sets, expected, monkeypatch, testing_lib, n):
    """BK_ITEM_GRID=2: two workgroups.  2047 and 2048 reads are 32 tiles, the two chunks the workgroups start with -- the edge just
    below; 2049 and 4097 are 33 and 65 tiles: a third chunk of one tile, and three more chunks, drawn from the launch's counter
    and handed over through the ring."""
    ix, _ = hpv
    eng = _engine_with(monkeypatch, ix, {"BK_ITEM_GRID": "2"})
    try:
        _sweep(oracle, expected, sets, ix, eng, "T %d" % n)
    finally:
        eng.close()


def _samples(mates, k, batch, times):
    return lambda e: [helpers.hip_sample(e, mates, k, batch=batch) for _ in range(times)]


@pytest.mark.parametrize("batch,times", [(513, 1), (None, 3)], ids=["two pushes", "three samples in a row"])
def test_set_t_over_pushes_and_samples(oracle, hpv, sets, expected, batch, times):
    """The deal's two counters take turns launch by launch and each launch zeroes the other's: two pushes in one sample, and
    samples in a row on one engine (both parities, either counter zeroed behind the other).  1025 reads: two workgroups."""
    ix, eng = hpv
    k, mates = sets["T 1025"]
    _sweep(oracle, expected, sets, ix, eng, "T 1025", run=_samples(mates, k, batch, times))


@pytest.mark.parametrize("env,n,batch,times", [({"BK_ITEM_GRID": "2"}, 4097, 2049, 3), ({"BK_MAX_LAUNCH_RECORDS": "700"}, 2049, None, 2)],
                         ids=["two workgroups: two pushes, three samples", "three launches a push, two samples"])
def test_set_t_over_launches_of_either_parity(oracle, hpv, sets, expected, monkeypatch, testing_lib, env, n, batch, times):
    """... with chunks drawn from the counter in every launch, and with pushes of an odd number of launches (700 records each), so
    that the same push starts on the other parity in the next sample."""
    ix, _ = hpv
    eng = _engine_with(monkeypatch, ix, env)
    k, mates = sets["T %d" % n]
    try:
        _sweep(oracle, expected, sets, ix, eng, "T %d" % n, run=_samples(mates, k, batch, times))
    finally:
        eng.close()
