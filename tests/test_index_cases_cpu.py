"""The cases of tests/index_cases.py without a GPU: the oracle's and the host's index builders (oracle.Index.build_mem,
HostIndex.build_mem) against the plain reference index_cases.expected() -- bucket ids, offsets and the entries byte for byte -- over
the very iterations that tests/test_gpu_index_fuzz.py runs through bk_build_index, and on every named case of at most MAX_PAIRS
pairs; on the larger named cases, where the oracle stands alone on the device side, the two builders against each other.  Then the
conditions that keep the fuzz from being vacuous, asserted on the reference's results alone and summed over those iterations."""
import functools

import numpy as np
import pytest

from tests import helpers, index_cases


@functools.lru_cache(maxsize=None)
def _fuzz(it):
    case = index_cases.make_case(index_cases.SEED, it)
    return (case,) + index_cases.reference(case)


def _arrays(ix):
    try:
        return ix.bucket_ids(), ix.bucket_off(), ix.entries()
    finally:
        ix.close()


def _builders(oracle, case):
    from bronko_amd.hostlib import HostIndex
    return (("oracle", _arrays(oracle.Index.build_mem(case.k, case.files))), ("host", _arrays(HostIndex.build_mem(case.k, case.files))))


def test_the_bucket_info_layout_is_the_products():
    from bronko_amd.engine import BUCKET_INFO_DTYPE
    assert index_cases.BUCKET_INFO_DTYPE == BUCKET_INFO_DTYPE and index_cases.BUCKET_INFO_DTYPE.itemsize == 12


@pytest.mark.parametrize("block", range(index_cases.BLOCKS))
def test_builders_equal_the_reference_on_the_fuzz(oracle, block):
    bad = []
    for it in range(block * index_cases.BLOCK, (block + 1) * index_cases.BLOCK):
        case, want, _ = _fuzz(it)
        assert index_cases.n_pairs(case.k, case.files) == len(want[2]) < index_cases.MAX_PAIRS, case.describe()
        for who, got in _builders(oracle, case):
            diff = index_cases.same(got, want)
            if diff:
                bad.append("%s: %s: %s" % (case.describe(), who, diff))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", index_cases.named_cases(), ids=lambda c: c.name)
def test_builders_on_the_named_cases(oracle, case):
    (_, orc), (_, host) = _builders(oracle, case)
    n = index_cases.n_pairs(case.k, case.files)
    assert len(orc[2]) == n
    if n <= index_cases.MAX_PAIRS:
        want = index_cases.expected(case.k, case.files)
        for who, got in (("oracle", orc), ("host", host)):
            diff = index_cases.same(got, want)
            assert diff is None, "%s: %s: %s" % (case.describe(), who, diff)
    else:
        diff = index_cases.same(host, orc)
        assert diff is None, "%s: host against oracle: %s" % (case.describe(), diff)
    # what the case is for, from the oracle's arrays
    ids, off, ent = orc
    sizes = np.diff(off.astype(np.int64))
    if case.name == "many_sequences":
        assert 255 in ent["seq_id"] and set(ent["file_id"].tolist()) == {0, 1} and set(ent["seq_id"][ent["file_id"] == 1].tolist()) == {0}
    elif case.name == "long_bucket":
        assert n == 1545390 and sizes.max() >= 140000
        assert sizes.max() >= 2 * (n / (n // index_cases.CHUNK + 1))        # chunks of the device build's host tail lie inside one bucket
    elif case.name == "deep_location":
        assert ent["location"].max() >= 1 << 16 and np.median(sizes) >= 60
        inside = np.ones(len(ent), bool)
        inside[off[:-1].astype(np.int64)] = False
        assert (np.diff(ent["location"].astype(np.int64))[inside[1:]] >= 0).all()   # one sequence: rising inside every bucket
    elif case.name == "identical_files":
        assert (sizes % 40 == 0).all() and set(ent["file_id"].tolist()) == set(range(40))
    elif case.name == "every_byte":
        assert len(set(case.files[0][1][0][1])) == 256
    elif case.name.startswith("lengths"):
        assert set(ent["seq_id"][ent["file_id"] == 0].tolist()) == {1, 2, 3, 4} and set(ent["seq_id"][ent["file_id"] == 6].tolist()) == {0, 1, 3, 4}
        assert set(ent["file_id"].tolist()) == {0, 2, 3, 5, 6}


def test_the_limits_of_the_host_builder():
    """257 sequences in a file are refused (seq_id is u8); 256 are taken (the named case)"""
    from bronko_amd.hostlib import HostIndex
    with pytest.raises(RuntimeError, match="256 sequences"):
        HostIndex.build_mem(21, index_cases.many_sequences_files(21, 257, np.random.default_rng(1)))


def test_a_case_is_a_function_of_seed_and_iteration():
    a, b = index_cases.make_case(7, 3), index_cases.make_case(7, 3)
    assert a.describe() == b.describe() and a.files == b.files and a.describe().startswith("fuzz seed=7 it=3 k=")
    assert index_cases.make_case(7, 4).files != a.files and index_cases.make_case(8, 3).files != a.files
    assert [c.files for c in index_cases.named_cases()] == [c.files for c in index_cases.named_cases()]


def test_the_fuzz_is_not_vacuous():
    t = {}
    for it in range(index_cases.BLOCKS * index_cases.BLOCK):
        case, _, walked = _fuzz(it)
        index_cases.tally(case, t, helpers.lcb_rank, walked)
    print(sorted(t.items()))
    assert t["iterations"] == 120
    for k in range(3, 32, 2):                                              # 1. every odd k
        assert t.get("k=%d" % k, 0) >= 1, (k, t)
    assert t.get("it_k31_rank_wraps", 0) >= 1, t                           # 2. at k = 31 an exact rank of 2^64 or more: the id wraps
    assert t["buckets_200_entries_3_files"] >= 10, t                       # 3. long buckets of several files
    for d in ("-1", "+0", "+1"):                                           # 4. k - 1, k and k + 1 bases as a file's last sequence
        assert t["it_last_sequence_of_k" + d] >= 1, (d, t)
    assert t["it_no_kmer"] >= 1, t                                         # 5. a case without any k-mer
    assert t["buckets_location_under_both_canonical"] >= 1, t              # 6. one location under both values of canonical
