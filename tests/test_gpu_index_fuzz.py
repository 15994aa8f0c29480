"""bk_build_index (bronko_amd/csrc/bk_build.hip) on the cases of tests/index_cases.py: the 120 random iterations against the plain
reference index_cases.expected(), the named cases against the oracle (which tests/test_index_cases_cpu.py holds to the same
reference wherever Python can) -- bucket ids, offsets, and the entries byte for byte.  Then its refusals, its empty results, 65,536
files with k-mers beyond gen_pairs_kernel's one grid trip, a build between two samples of a live engine, engines created on
device-built indexes, and `bronko build` on the device against the same command on the host."""
import functools
import os
import subprocess
import time

import numpy as np
import pytest

from bronko_amd import BronkoError, Engine, build_index_device
from tests import helpers, index_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
BK_ERR_INVALID, BK_ERR_NO_DEVICE = -1, -2


@functools.lru_cache(maxsize=None)
def _case(it):
    return index_cases.make_case(index_cases.SEED, it)


@functools.lru_cache(maxsize=None)
def _fuzz(it):
    """(case, expected) of iteration `it`; computed once, shared, never written to"""
    case = _case(it)
    return case, index_cases.expected(case.k, case.files)


def _oracle_arrays(oracle, k, files):
    ix = oracle.Index.build_mem(k, files)
    try:
        return ix.bucket_ids(), ix.bucket_off(), ix.entries()
    finally:
        ix.close()


@pytest.mark.parametrize("block", range(index_cases.BLOCKS))
def test_device_build_equals_the_reference_on_the_fuzz(block):
    bad = []
    for it in range(block * index_cases.BLOCK, (block + 1) * index_cases.BLOCK):
        case, want = _fuzz(it)
        diff = index_cases.same(build_index_device(case.k, case.files), want)
        if diff:
            bad.append("%s: %s" % (case.describe(), diff))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", index_cases.named_cases(), ids=lambda c: c.name)
def test_device_build_equals_the_oracle_on_the_named_cases(oracle, case):
    want = _oracle_arrays(oracle, case.k, case.files)
    got = build_index_device(case.k, case.files)
    diff = index_cases.same(got, want)
    assert diff is None, "%s: %s" % (case.describe(), diff)
    assert len(got[2]) == index_cases.n_pairs(case.k, case.files)
    sizes = np.diff(want[1].astype(np.int64))
    if case.name == "many_sequences":
        assert 255 in got[2]["seq_id"] and set(got[2]["file_id"].tolist()) == {0, 1}
    elif case.name == "long_bucket":                                       # from the expected offsets alone
        n = int(want[1][-1])
        assert n == 1545390 and sizes.max() >= 2 * (n / (n // index_cases.CHUNK + 1))
    elif case.name == "deep_location":
        assert got[2]["location"].max() >= 1 << 16


def _refused(status, k, files, device=0):
    with pytest.raises(BronkoError) as e:
        build_index_device(k, files, device)
    assert e.value.status == status, e.value
    message = str(e.value).split(": ", 1)[1]                               # bk_build_last_error()
    assert message.strip(), e.value
    return message


def test_refusals():
    g = index_cases.rand_seq(np.random.default_rng(1), 100)
    one = [("f", [("s", g)])]
    for k in (1, 20, 33):
        assert "kmer size" in _refused(BK_ERR_INVALID, k, one)
    assert "256 sequences" in _refused(BK_ERR_INVALID, 21, index_cases.many_sequences_files(21, 257, np.random.default_rng(2)))
    assert "n_files" in _refused(BK_ERR_INVALID, 21, one + [("e", [])] * 65536)
    _refused(BK_ERR_NO_DEVICE, 21, one, device=99)
    # ... and the next call is served
    ids, off, ent = build_index_device(21, one)
    assert len(ent) == 80 * 21 and off[-1] == len(ent)


@pytest.mark.parametrize("files", [[], [("a", [("e", b"")]), ("b", [("e0", b""), ("e1", b"")])],
                                   [("a", [("s", b"ACGTACGTAC"), ("t", b"A")]), ("b", []), ("c", [("u", b"ACGTACGTACGTACGTACGT")])]],
                         ids=["no_files", "empty_sequences", "all_shorter_than_k"])
def test_empty_results(files):
    ids, off, ent = build_index_device(21, files)
    assert len(ids) == 0 and off.tolist() == [0] and len(ent) == 0 and ent.dtype == index_cases.BUCKET_INFO_DTYPE


def test_65536_files_and_the_second_grid_trip(oracle):
    """65,536 files of the same three sequences of 130, 2 and 131 bases at k = 3: 257 k-mers a file, 16,842,752 in all -- 65,536 past
    the 16,777,216 threads of gen_pairs_kernel's one trip -- and 50.5 M pairs.  Expected: the oracle's index of one file, every
    bucket's list repeated per file with file_id = f (build.rs:223-228 appends the files' lists in file order)."""
    t0 = time.time()
    rng = np.random.default_rng((index_cases.SEED, 65536))
    F, k = 65536, 3
    three = [("a", index_cases.rand_seq(rng, 130)), ("b", index_cases.rand_seq(rng, 2)), ("c", index_cases.rand_seq(rng, 131))]
    ids1, off1, ent1 = _oracle_arrays(oracle, k, [("one", three)])
    per_file = len(ent1)
    assert per_file == 257 * k and 257 * F == (1 << 24) + 65536
    want = np.zeros(per_file * F, index_cases.BUCKET_INFO_DTYPE)           # (zeroed: the padding bytes are compared)
    o1 = off1.astype(np.int64)
    for b in range(len(ids1)):
        seg = want[o1[b] * F:o1[b + 1] * F].reshape(F, -1)
        for name in ("seq_id", "location", "idx", "canonical"):
            seg[name] = ent1[name][o1[b]:o1[b + 1]][None, :]
        seg["file_id"] = np.arange(F, dtype=np.uint16)[:, None]
    ids, off, ent = build_index_device(k, [("f", three)] * F)
    assert np.array_equal(ids, ids1) and np.array_equal(off, off1 * np.uint64(F))
    assert ent.dtype == want.dtype and len(ent) == len(want)
    assert 65535 in ent["file_id"]
    # the files from 65,280 upwards hold the k-mers of the second trip: all their entries are there ...
    # (rows of bytes are picked, not records: picking records leaves the copies' padding bytes undefined)
    got_b, want_b = ent.view(np.uint8).reshape(-1, 12), want.view(np.uint8).reshape(-1, 12)
    late, late_want = got_b[ent["file_id"] >= 65280], want_b[want["file_id"] >= 65280]
    assert len(late) == 256 * per_file and np.array_equal(late, late_want)
    # ... and everything else
    assert np.array_equal(got_b, want_b)
    print("65,536 files: %d pairs, %.1f s" % (len(ent), time.time() - t0))


def test_a_build_between_two_samples_of_a_live_engine(oracle, golden_dir):
    """The build has a stream, buffers and a hipSetDevice of its own: an engine with a finished sample behind it and another ahead
    is not disturbed by four builds in between, nor they by it."""
    ix = oracle.Index.load(os.path.join(golden_dir, "hpv.bkdb"))
    eng = helpers.engine_from_oracle_index(ix)
    try:
        reads = helpers.hpv_reads(3000, seed=11)
        helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), oracle.sample_pileup(ix, [reads]))
        for it in (3, 33, 63, 93):
            case, want = _fuzz(it)
            diff = index_cases.same(build_index_device(case.k, case.files), want)
            assert diff is None, "%s: %s" % (case.describe(), diff)
        reads = helpers.hpv_reads(3000, seed=12, with_n=True)
        helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], 21), oracle.sample_pileup(ix, [reads]))
    finally:
        eng.close()
        ix.close()


def _engine_cases():
    """Six iterations with k >= 11 whose first file holds a sequence of 100 bases or more: the first two at k = 31 with three or more
    files, and the first four at another k"""
    k31, rest = [], []
    for it in range(index_cases.BLOCKS * index_cases.BLOCK):
        case = _case(it)
        if case.k < 11 or not case.files[0][1] or max(len(s) for _, s in case.files[0][1]) < 100:
            continue
        if case.k == 31 and len(case.files) >= 3 and len(k31) < 2:
            k31.append(it)
        elif case.k < 31 and len(rest) < 4:
            rest.append(it)
    assert len(k31) == 2 and len(rest) == 4
    return k31 + rest


@pytest.mark.parametrize("it", _engine_cases())
def test_an_engine_on_a_device_built_index(oracle, it):
    """bk_engine_create checks every bucket against assign_buckets of its own entries -- a second judge of the arrays -- and a sample
    of 300 reads cut from the case's first file maps as on the oracle's index."""
    case, want = _fuzz(it)
    ids, off, ent = build_index_device(case.k, case.files)
    assert index_cases.same((ids, off, ent), want) is None, case.describe()
    rng = np.random.default_rng((index_cases.SEED, it, 2))
    src = max((s for _, s in case.files[0][1]), key=len)
    reads = []
    for _ in range(300):
        n = int(rng.integers(min(len(src), 40), min(len(src), 150) + 1))
        a = int(rng.integers(0, len(src) - n + 1))
        r = src[a:a + n]
        reads.append(index_cases.revcomp(r) if rng.random() < 0.5 else r)
    ix = oracle.Index.build_mem(case.k, case.files)
    eng = None
    try:
        eng = Engine(case.k, ids, off, ent, case.files)
        pile = oracle.sample_pileup(ix, [reads])
        assert int(pile.fwd_nk.sum() + pile.rev_nk.sum()) > 0, case.describe()     # (the sample does map)
        helpers.assert_same_pileup(helpers.hip_sample(eng, [reads], case.k), pile)
    finally:
        if eng is not None:
            eng.close()
        ix.close()


def test_an_engine_on_files_without_sequences_between_others(oracle):
    """A file without sequences, and one of sequences shorter than k only, between files that hold k-mers (the named case
    lengths[21]): bk_engine_create once gave such a file the cells of every file behind it and never returned.  Reads of the last
    file map as on the oracle's index, with every genome's rows and with the selected genome's only."""
    from bronko_amd import Params
    from tests import level_sweep
    case = [c for c in index_cases.named_cases() if c.name == "lengths[21]"][0]
    assert [len(recs) for _, recs in case.files][4] == 0 and case.files[-1][1]
    ids, off, ent = build_index_device(case.k, case.files)
    src = case.files[-1][1][1][1]
    reads = [src[a:a + 50] for a in range(0, len(src) - 50 + 1)] * 3
    ix = oracle.Index.build_mem(case.k, case.files)
    pile = oracle.sample_pileup(ix, [reads])
    assert int(pile.fwd_nk.sum()) > 0 and oracle.pick_best_genome(ix, pile.stats.sum(axis=0), pile.present.max(axis=0)) == len(case.files) - 1
    try:
        for params in (None, Params(pileup_selected_only=True)):
            eng = Engine(case.k, ids, off, ent, case.files, params)
            try:
                level_sweep.assert_same_level(oracle, ix, helpers.hip_sample(eng, [reads], case.k), pile, selected_only=params is not None)
            finally:
                eng.close()
    finally:
        ix.close()


def _cli_cases():
    """the first three iterations with k >= 15 and at least one k-mer"""
    out = []
    for it in range(index_cases.BLOCKS * index_cases.BLOCK):
        case = _case(it)
        if case.k >= 15 and index_cases.n_pairs(case.k, case.files) > 0 and len(out) < 3:
            out.append(it)
    return out


@pytest.mark.parametrize("it", _cli_cases())
def test_bronko_build_writes_the_same_index_on_the_device_and_on_the_host(oracle, tmp_path, it):
    case, want = _fuzz(it)
    paths = []
    for name, recs in case.files:
        paths.append(str(tmp_path / (name + ".fa")))
        with open(paths[-1], "wb") as f:
            for sname, seq in recs:
                f.write(b">" + sname.encode() + b" a comment\n")
                for a in range(0, len(seq), 70):
                    f.write(seq[a:a + 70] + b"\n")
    out = {}
    for how, env in (("device", {}), ("host", {"BRONKO_BUILD_ON_HOST": "1"})):
        stem = str(tmp_path / how)
        env = {**{n: v for n, v in os.environ.items() if n != "BRONKO_BUILD_ON_HOST"}, **env}
        res = subprocess.run([BRONKO, "build", "-g"] + paths + ["-k", str(case.k), "-o", stem, "--verbose"], capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        # without this line the device path did not run, and the comparison below would prove nothing
        assert ("index built on the GPU" in res.stdout + res.stderr) == (how == "device"), res.stdout + res.stderr
        out[how] = open(stem + ".bkdb", "rb").read()
    assert out["device"] == out["host"], case.describe()
    built = oracle.Index.build(case.k, paths)
    loaded = oracle.Index.load(str(tmp_path / "device.bkdb"))
    try:
        got = (loaded.bucket_ids(), loaded.bucket_off(), loaded.entries())
        diff = index_cases.same(got, (built.bucket_ids(), built.bucket_off(), built.entries()))
        assert diff is None, "%s: %s" % (case.describe(), diff)
        assert index_cases.same(got, want) is None, case.describe()
        assert loaded.k == built.k == case.k and loaded.files() == built.files()
        assert [(n, [s for _, s in recs]) for n, recs in loaded.files()] == [(n, [s for _, s in recs]) for n, recs in case.files]
    finally:
        built.close()
        loaded.close()
