"""bk_sample_call on crafted pileups (tests/pileup_cases.py): the device caller's walk, strip and call filters where simulated reads
never take them -- frequencies within 1e-12 of each other, tables that drain and refill, lists of states at their allowance, many
sequences per genome behind another genome's cells, every filter at its threshold -- against the oracle, which
tests/test_caller_ref_cpu.py holds against an independent restatement on the same pileups.

The way in: a sample of ~200 error-free reads of the target genome is finalized (only so that the statistics select it), the
device pileup is overwritten with the crafted arrays, then bk_sample_call runs on it."""
import numpy as np
import pytest

from tests import helpers, pileup_cases

pytestmark = pytest.mark.gpu
K = pileup_cases.K


class _Bench:
    """Engines and oracle indexes by layout, made inside the test (so that they bind the library the test asked for)."""

    def __init__(self, oracle):
        self.oracle, self.by_layout = oracle, {}

    def get(self, lay):
        if lay.name not in self.by_layout:
            ix = self.oracle.Index.build_mem(K, lay.files)
            self.by_layout[lay.name] = (ix, helpers.engine_from_oracle_index(ix))
        return self.by_layout[lay.name]

    def close(self):
        for ix, eng in self.by_layout.values():
            eng.close()
            ix.close()


def _call(oracle, ix, eng, case):
    """One case through bk_sample_call and the comparison of tests/test_gpu_calls.py; returns (positions, records) compared."""
    import torch
    from bronko_amd import pack_reads
    from bronko_amd.dist import DeviceVector
    lay = case.layout
    eng.sample_begin()
    words, lens = pack_reads(lay.selection_reads(), K)
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    res = eng.sample_download(1, arrays=False)
    best = oracle.pick_best_genome(ix, res.stats.sum(axis=0), res.present.max(axis=0))
    assert best == lay.target, "%s: the reads select genome %d" % (case.name, best)
    cells4 = eng.total_cells * 4
    assert cells4 == len(case.fwd)
    dev = torch.as_tensor(DeviceVector(eng.pileup_ptr(), 4 * cells4), device="cuda:0")
    dev.copy_(torch.from_numpy(np.concatenate(case.arrays()).view(np.int64)))
    torch.cuda.synchronize()
    eng.sample_call(1, case.params.apply(eng.call_params()))
    pile = oracle.Pileup(ix)
    pile.fwd_depth[:], pile.rev_depth[:], pile.fwd_nk[:], pile.rev_nk[:] = case.arrays()
    op = case.params.apply(oracle.default_call_params(K))
    try:
        n = helpers.assert_same_calls(oracle, ix, eng, pile, best, op)
    except AssertionError as e:
        raise AssertionError("case %s: %s" % (case.name, e)) from e
    return sum(n_pos for _, n_pos in lay.seqs), n


def _run_all(oracle, cases):
    bench = _Bench(oracle)
    totals = {}
    try:
        for case in cases:
            ix, eng = bench.get(case.layout)
            p, r = _call(oracle, ix, eng, case)
            t = totals.setdefault(case.family, [0, 0, 0])
            t[0], t[1], t[2] = t[0] + 1, t[1] + p, t[2] + r
    finally:
        bench.close()
    for family, (n, p, r) in sorted(totals.items()):
        print("%-12s %3d cases, %7d positions, %6d records compared" % (family, n, p, r))
    return totals


def test_named_cases_split_walk(oracle):
    totals = _run_all(oracle, pileup_cases.named_cases())
    assert set(totals) == {"lengths", "near_ties", "exact_ties", "table_life", "three_ranks", "strip", "filters", "selection"}
    assert totals["filters"][2] > 100 and totals["near_ties"][2] > 0


def test_named_cases_walk_in_one_wave(oracle, monkeypatch, testing_lib):
    monkeypatch.setenv("BK_NOISE_SERIAL", "1")
    _run_all(oracle, pileup_cases.named_cases())


def test_random_mix_split_walk(oracle):
    cases, _ = pileup_cases.random_mix(200)
    assert _run_all(oracle, cases)["random"][2] > 2000


def test_random_mix_walk_in_one_wave(oracle, monkeypatch, testing_lib):
    monkeypatch.setenv("BK_NOISE_SERIAL", "1")
    cases, _ = pileup_cases.random_mix(200)
    _run_all(oracle, cases)


def test_two_samples_in_a_row_and_on_a_fork(oracle):
    """A case that fills the lists of table states, then a sparse one on the same engine -- what the first left in noise_tbl and
    noise_state must not show --, then the same pair on a fork of that engine, and once more on the engine itself."""
    by = {c.name: c for c in pileup_cases.named_cases()}
    heavy, sparse = by["table_increasing"], by["lengths_sparse"]
    assert heavy.layout is sparse.layout
    ix = oracle.Index.build_mem(K, heavy.layout.files)
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    try:
        for e in (eng, fork, eng):
            _call(oracle, ix, e, heavy)
            _call(oracle, ix, e, sparse)
            _call(oracle, ix, e, by["table_decreasing"])
            _call(oracle, ix, e, sparse)
    finally:
        fork.close()
        eng.close()
        ix.close()


def test_selection_tie_takes_the_lowest_id(oracle):
    """Two genome files with the same sequences: the statistics tie, pick_best_genome's strict > keeps the first (call.rs:443)."""
    case = pileup_cases.tie_case()
    assert case.layout.target == 0 and case.layout.files[0][1][0][1] == case.layout.files[1][1][0][1]
    ix = oracle.Index.build_mem(K, case.layout.files)
    eng = helpers.engine_from_oracle_index(ix)
    try:
        _call(oracle, ix, eng, case)
        summ, _ = eng.download_calls()
        assert summ.file_id == 0
        res = eng.sample_download(1, arrays=False)
        assert res.present[0].tolist() == [1, 1] and res.stats[0, 0].tolist() == res.stats[0, 1].tolist() and res.stats[0, 0, 0] > 0
    finally:
        eng.close()
        ix.close()
