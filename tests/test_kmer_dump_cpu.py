"""--keep-kmer-info without a GPU: the host writer of <stem>_counts.txt, and the bk_kmer_dump_* entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

from bronko_amd import _ffi, hostlib
from tests import helpers


@pytest.mark.parametrize("k", [3, 31])
@pytest.mark.parametrize("threads", [1, 3, 8])
def test_write_kmer_counts_matches_python(tmp_path, k, threads):
    rng = np.random.default_rng(k * 100 + threads)
    n = 200000 if k == 31 else 64
    km = np.sort(rng.integers(0, 1 << (2 * k), n, dtype=np.uint64))
    ct = rng.integers(1, 1000001, n, dtype=np.uint64)
    ct[:3] = [1, 10, 1000000]
    path = str(tmp_path / "x_counts.txt")
    hostlib.write_kmer_counts(path, k, km, ct, threads)
    want = "".join("%s\t%d\n" % (helpers.kmer_str(int(v), k), int(c)) for v, c in zip(km, ct)).encode()
    assert open(path, "rb").read() == want


def test_write_kmer_counts_empty(tmp_path):
    path = str(tmp_path / "e_counts.txt")
    hostlib.write_kmer_counts(path, 21, np.zeros(0, np.uint64), np.zeros(0, np.uint64), 4)
    assert open(path, "rb").read() == b""


def test_write_kmer_counts_unwritable_path(tmp_path):
    with pytest.raises(RuntimeError):
        hostlib.write_kmer_counts(str(tmp_path / "no" / "such" / "dir.txt"), 21, np.zeros(1, np.uint64), np.ones(1, np.uint64), 1)


@pytest.mark.parametrize("testing", [False, True])
def test_dump_entry_points_refuse_a_null_engine(testing):
    L = _ffi.load(testing=testing)
    for s in ("bk_kmer_dump_enable", "bk_kmer_dump_size", "bk_kmer_dump_download"):
        assert hasattr(L, s), s
    kept, distinct = C.c_uint64(), C.c_uint64()
    buf = (C.c_uint64 * 4)()
    assert L.bk_kmer_dump_enable(None, 20) == -1
    assert L.bk_kmer_dump_enable(None, 0) == -1
    assert L.bk_kmer_dump_size(None, 0, C.byref(kept), C.byref(distinct)) == -1
    assert L.bk_kmer_dump_download(None, 0, buf, buf, 4) == -1
