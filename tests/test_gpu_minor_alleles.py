"""bk_sample_minor_alleles (minor_alleles_kernel) against the plain-numpy restatement (tests/contamination_ref.py) on the crafted
pileups of tests/consensus_ref.py, put on the device the way tests/test_gpu_consensus.py does it; the call order and parameter checks
of the C ABI; a sample that selects no genome."""
import ctypes as C

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads
from tests import consensus_ref, contamination_ref, helpers, pileup_cases
from tests.test_gpu_consensus import _Engines, _to_call

pytestmark = pytest.mark.gpu
K = pileup_cases.K
# (R, F) with exact-threshold cells in the crafted pileups: counts of 10 and 9 (tot == R, tot == R - 1), 225 / 75 and 50 / 50 and
# 150 / 100 / 50 (tot == F x depth at F = 0.25 and 0.5), F = 0 and F = 1
PARAMS = [(10, 0.03), (10, 0.0), (1, 0.25), (1, 0.5), (1, 1.0), (20, 0.25), (300, 0.5)]


def _expected(case, r, f):
    """The restatement over the target genome's sequences in their order, computed once and kept with the case."""
    kept = case.__dict__.setdefault("_minor_ref", {})
    if (r, f) not in kept:
        masks, t = [], dict.fromkeys(contamination_ref.TALLIES, 0)
        for cell0, length in case.layout.seqs:
            m, ts = contamination_ref.present_masks(case.fwd[cell0 * 4:(cell0 + length) * 4], case.rev[cell0 * 4:(cell0 + length) * 4], r, f)
            masks.append(m)
            for k in t:
                t[k] += ts[k]
        kept[(r, f)] = (np.concatenate(masks), t)
    return kept[(r, f)]


def _check(eng, case):
    _to_call(eng, case)
    n = 0
    for r, f in PARAMS:
        want, want_t = _expected(case, r, f)
        eng.sample_minor_alleles(eng.minor_params(min_reads=r, min_freq=f))
        summ, masks = eng.download_minor_alleles()
        assert summ.file_id == case.layout.target, case.name
        assert {k: getattr(summ, k) for k in contamination_ref.TALLIES} == want_t, (case.name, r, f)
        bad = np.flatnonzero(masks != want)
        assert not len(bad), "%s at R = %d, F = %r: %d masks differ, first at %d: %d, expected %d" % (case.name, r, f, len(bad), bad[0], masks[bad[0]], want[bad[0]])
        n += len(masks)
    return n


def test_crafted_cases(oracle):
    cases = consensus_ref.crafted_cases()
    seen = set()
    for case in cases:                                           # the thresholds are met exactly somewhere, and missed by one
        for r, f in PARAMS:
            seen.update(_expected(case, r, f)[0].tolist())
    assert seen == set(range(16))
    engines, n = _Engines(oracle), 0
    try:
        for case in cases:
            n += _check(engines.get(case.layout), case)
    finally:
        engines.close()
    assert n > 7 * 10000


def test_two_samples_in_a_row_and_on_a_fork_beside_the_consensus(oracle):
    """Masks and tallies of the sample before must not show; the consensus of the same sample is what it is without the masks."""
    by = {c.name: c for c in consensus_ref.named_cases()}
    heavy, sparse = by["table_increasing"], by["lengths_sparse"]
    short = [c for c in consensus_ref.crafted_cases() if c.name == "consensus_short_genome"][0]
    ix = oracle.Index.build_mem(K, heavy.layout.files)
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    try:
        for e in (eng, fork, eng):
            for case in (heavy, short, sparse):
                _check(e, case)
                e.sample_consensus()
                want_letters, want = consensus_ref.expected(case, 10, 0.5)
                summ, letters = e.download_consensus()
                assert letters == want_letters and {k: getattr(summ, k) for k in consensus_ref.TALLIES} == want
                want_m, _ = _expected(case, 10, 0.03)            # ... and the masks made before it are still there
                e.sample_minor_alleles()
                assert np.array_equal(e.download_minor_alleles()[1], want_m)
    finally:
        fork.close()
        eng.close()
        ix.close()


def test_call_order_parameters_and_cap(oracle):
    case = [c for c in consensus_ref.crafted_cases() if c.name == "consensus_rule"][0]
    lay = case.layout
    ix = oracle.Index.build_mem(K, lay.files)
    eng = helpers.engine_from_oracle_index(ix)

    def status(fn, *a):
        with pytest.raises(BronkoError) as ei:
            fn(*a)
        return ei.value.status, str(ei.value)

    try:
        assert status(eng.sample_minor_alleles)[0] == -5         # BK_ERR_STATE: nothing was ever called
        eng.sample_begin()
        assert status(eng.sample_minor_alleles)[0] == -5         # inside a sample
        words, lens = pack_reads(lay.selection_reads(), K)
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        assert status(eng.sample_minor_alleles)[0] == -5         # finalized, but not called
        assert status(eng.download_minor_alleles)[0] == -5
        _to_call(eng, case)
        assert status(eng.download_minor_alleles)[0] == -5       # called, but no masks made
        st, msg = status(eng.sample_minor_alleles, eng.minor_params(min_reads=0))
        assert st == -1 and "min_reads" in msg                  # BK_ERR_INVALID, the parameter named
        for bad in (1.5, -0.1, float("nan")):
            st, msg = status(eng.sample_minor_alleles, eng.minor_params(min_freq=bad))
            assert st == -1 and "min_freq" in msg
        p = eng.minor_params()
        assert (p.min_reads, p.min_freq) == (10, 0.03)
        eng.sample_minor_alleles()
        want, want_t = _expected(case, 10, 0.03)
        summ, masks = eng.download_minor_alleles(cap=100)        # fewer than the genome has: `cap` bytes, the full count
        assert summ.positions == len(want) > 100 and np.array_equal(masks, want[:100])
        raw, rs = np.full(200, 0xff, np.uint8), _ffi.MinorSummary()   # ... and nothing behind them is written
        assert eng._L.bk_sample_download_minor_alleles(eng.h, C.byref(rs), raw.ctypes.data_as(C.c_void_p), 100) == 0
        assert np.array_equal(raw[:100], want[:100]) and (raw[100:] == 0xff).all() and rs.positions == len(want)
        assert np.array_equal(eng.download_minor_alleles(cap=len(want) + 50)[1], want)
        eng.sample_begin()                                       # the next sample: the masks are no longer this sample's
        assert status(eng.sample_minor_alleles)[0] == -5
        assert status(eng.download_minor_alleles)[0] == -5
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        eng.sample_call(1)
        assert status(eng.download_minor_alleles)[0] == -5       # ... not before its own bk_sample_minor_alleles
        eng.sample_minor_alleles()
        assert eng.download_minor_alleles()[0].file_id == lay.target
    finally:
        eng.close()
        ix.close()


def test_no_genome_selected(oracle):
    """A sample without reads selects nothing: file_id -1, every tally 0, no bytes."""
    lay = pileup_cases.layout("multi")
    ix = oracle.Index.build_mem(K, lay.files)
    eng = helpers.engine_from_oracle_index(ix)
    try:
        eng.sample_begin()
        eng.sample_finalize(1)
        eng.sample_call(1)
        eng.sample_minor_alleles()
        summ, masks = eng.download_minor_alleles()
        assert summ.file_id == -1 and len(masks) == 0
        assert [getattr(summ, k) for k in contamination_ref.TALLIES] == [0, 0, 0]
    finally:
        eng.close()
        ix.close()
