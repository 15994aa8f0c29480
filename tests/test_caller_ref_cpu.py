"""The stages after the pileup on crafted pileups (tests/pileup_cases.py), three ways on the CPU: the plain-Python restatement
written from upstream's text (tests/caller_ref.py), the oracle (oracle/bronko_oracle.c) and the product's host caller
(bronko_amd/host/caller.cpp).  The oracle and the host caller share one reading of call.rs with the device caller; the Python
restatement does not, and the pileups are made to reach what simulated reads never do (see pileup_cases)."""
import numpy as np
import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import caller_ref, pileup_cases

NAMED = pileup_cases.named_cases()
_indexes = {}


def _index(oracle, lay):
    if lay.name not in _indexes:
        _indexes[lay.name] = (oracle.Index.build_mem(pileup_cases.K, lay.files), HostIndex.build_mem(pileup_cases.K, lay.files))
    return _indexes[lay.name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b, nan_ok=False):
    """bit for bit; nan_ok: a NaN equals a NaN whatever its sign (sqrt of a negative number: the sign of the NaN is the platform's)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = _bits(a) == _bits(b)
    if nan_ok:
        same |= np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(same.all())


def _check(oracle, case, tmp_path):
    """One case through the three; returns (positions compared, records compared)."""
    lay = case.layout
    oix, hix = _index(oracle, lay)
    assert oix.total_cells == lay.total_cells and [oix.cell_offset(lay.target, s) for s in range(len(lay.seqs))] == [c for c, _ in lay.seqs]
    pile = oracle.Pileup(oix)
    pile.fwd_depth[:], pile.rev_depth[:], pile.fwd_nk[:], pile.rev_nk[:] = case.arrays()
    recs, summ, noise, _ = pileup_cases.reference(case)
    # ---- noise: max, mean, std against the oracle, max against the host caller
    for (c0, n), (rmax, rmean, rstd) in zip(lay.seqs, noise):
        f4, r4 = case.fwd[c0 * 4:(c0 + n) * 4], case.rev[c0 * 4:(c0 + n) * 4]
        omax, omean, ostd = oracle.baseline_noise(f4, r4)
        assert _same_bits(rmax, omax), "%s: Noise.max differs from the oracle's at %s" % (case.name, np.nonzero(_bits(rmax) != _bits(omax))[0][:5])
        assert _same_bits(rmean, omean, nan_ok=True) and _same_bits(rstd, ostd, nan_ok=True), case.name
        hmax = hostlib.baseline_noise_max(f4, r4)
        assert _same_bits(rmax, hmax), "%s: Noise.max differs from the host caller's at %s" % (case.name, np.nonzero(_bits(rmax) != _bits(hmax))[0][:5])
    # ---- records and summary against the oracle
    op = case.params.apply(oracle.default_call_params(pileup_cases.K))
    orecs, optr, n, nmaj, nmin, breadth, depth = oracle.call_variants(oix, lay.target, pile, op)
    try:
        assert (len(recs), summ[0], summ[1]) == (n, nmaj, nmin), case.name
        for r, o in zip(recs, orecs):
            for name in ("seq_id", "pos", "ref_base", "alt_base", "fwd_ref", "rev_ref", "fwd_alt", "rev_alt", "depth"):
                assert r[name] == o[name], (case.name, name, r, o)
            assert _same_bits([r["af"]], [o["af"]]), (case.name, r, o)
            assert abs(r["sor"] - o["sor"]) <= 1e-12 * max(1.0, abs(o["sor"])), (case.name, r, o)
            assert "%.3f" % r["sor"] == "%.3f" % o["sor"]
        rb, rd = caller_ref.coverage(summ)
        assert _same_bits([rb], [breadth], nan_ok=True) and _same_bits([rd], [depth], nan_ok=True), case.name
        # ---- the host caller's files against the oracle's writers, byte for byte
        o_vcf, o_tsv, h_vcf, h_tsv = (str(tmp_path / f) for f in ("o.vcf", "o.tsv", "h.vcf", "h.tsv"))
        oracle.write_vcf(o_vcf, "dir/crafted_R1.fastq.gz", oix, lay.target, optr, n)
        oracle.write_pileup(o_tsv, oix, lay.target, pile)
        hp = case.params.apply(hostlib.default_call_params(pileup_cases.K))
        hn, hmaj, hmin, hbr, hdc = hostlib.call_and_write(hix, lay.target, case.arrays(), hp, h_vcf, "dir/crafted_R1.fastq.gz", h_tsv)
        assert (hn, hmaj, hmin) == (n, nmaj, nmin), case.name
        assert _same_bits([hbr], [breadth], nan_ok=True) and _same_bits([hdc], [depth], nan_ok=True)
        with open(h_vcf, "rb") as a, open(o_vcf, "rb") as b:
            assert a.read() == b.read(), case.name
        with open(h_tsv, "rb") as a, open(o_tsv, "rb") as b:
            assert a.read() == b.read(), case.name
    finally:
        oracle.lib().orc_free(optr)
    return sum(n for _, n in lay.seqs), len(recs)


def _trace(case, s=0, **kw):
    c0, n = case.layout.seqs[s]
    tr = []
    out = caller_ref.baseline_noise(case.fwd[c0 * 4:(c0 + n) * 4], case.rev[c0 * 4:(c0 + n) * 4], trace=tr, **kw)
    return out, tr


@pytest.mark.parametrize("case", NAMED, ids=[c.name for c in NAMED])
def test_named_case(oracle, tmp_path, case):
    assert case.layout.total_cells <= 10000
    # no named case sits within 1e-9 of a decision that goes through ln() or pow(): none needs a nudge, none loses its edge to one
    assert pileup_cases.too_close(case) == []
    positions, records = _check(oracle, case, tmp_path)
    print("%s: %d positions, %d records compared" % (case.name, positions, records))


def test_random_mix(oracle, tmp_path):
    cases, redrawn = pileup_cases.random_mix(200)
    assert len(cases) == 200 and redrawn <= 2                   # at most 1 % drawn again for a decision too close to its threshold
    assert all(pileup_cases.too_close(c) == [] for c in cases)
    positions = records = 0
    for c in cases:
        p, r = _check(oracle, c, tmp_path)
        positions, records = positions + p, records + r
    assert records > 2000 and len({c.layout.name for c in cases}) == 3
    print("random mix: %d positions, %d records compared, %d nudges, %d redrawn" % (positions, records, sum(c.nudges for c in cases), redrawn))


def test_eviction_canary():
    """The walk with its eviction by equality instead of `< 1e-12` must give another Noise.max on the near-tie cases (else they say
    nothing about the rule) and the same on the exact ties (where the two rules agree)."""
    for case in NAMED:
        if case.family not in ("near_ties", "exact_ties"):
            continue
        (want, _, _), _ = _trace(case)
        (got, _, _), _ = _trace(case, evict_exact=True)
        differ = int((_bits(want) != _bits(got)).sum())
        print("%s: eviction by equality differs at %d positions" % (case.name, differ))
        assert (differ > 0) == (case.family == "near_ties"), (case.name, differ)


def test_cases_reach_what_they_are_for():
    """The crafted windows do occur: n = 1, 2, 3 and 300, seven entries stripped, a table that drains, sequences shorter than a
    window, and the filter case reports exactly the edits upstream's rules let through."""
    by = {c.name: c for c in NAMED}
    ns = {n for n, _ in _trace(by["strip_n_1_2_3"])[1]}
    assert {0, 1, 2, 3} <= ns
    assert max(n for n, _ in _trace(by["strip_n_300"])[1]) == 300
    assert max(cur for _, cur in _trace(by["strip_seven"])[1]) == 7
    assert max(cur for _, cur in _trace(by["strip_outlier"])[1]) >= 1
    tr = _trace(by["table_drain_refill"])[1]
    assert any(n == 0 for n, _ in tr[150:390]) and all(n > 0 for n, _ in tr[:100]) and all(n > 0 for n, _ in tr[450:])
    assert max(n for n, _ in _trace(by["table_never_fills"])[1]) < caller_ref.TABLE
    assert sorted(n for _, n in by["lengths"].layout.seqs) == sorted(pileup_cases.LENGTHS) and by["lengths"].layout.seqs[0][0] != 0
    # filters_default: slots 0-4 (every reference letter), 5 (one strand, SOR 4.8), 8, 9 (af = min_af), 11 (af = 1/2), 13 (depth 300),
    # 15 (depth 300), 17-19 (k-mer support 2 on a strand), 20, 22 (2^40); position k of sequence 0, len - k - 1 of sequences 1 and 2,
    # k of sequence 3.  Not: 6, 7 (SOR), 10 (af), 12, 14 (depth 299), 16 (support 1 / 1), 21 (three equal alleles: the second is the
    # noise level), 23, 24 (af), k - 1 and len - k, sequences of 2k positions and fewer.
    K, L = pileup_cases.K, pileup_cases.FILTER_LENS
    want = [(0, K)] + [(0, 140 + 105 * j) for j in (0, 1, 2, 3, 4, 5, 8, 9, 11, 13, 15, 17, 18, 19, 20, 22)] + \
           [(1, L[1] - K - 1), (2, L[2] - K - 1), (3, K)]
    recs = pileup_cases.reference(by["filters_default"])[0]
    assert [(r["seq_id"], r["pos"] - 1) for r in recs] == sorted(want)
    assert [r for r in recs if r["af"] >= 0.5] == [r for r in recs if r["pos"] - 1 == 140 + 105 * 11] and len(recs) == 20
    loose = pileup_cases.reference(by["filters_loose"])[0]
    assert sum(1 for r in loose if r["pos"] - 1 == 140 + 105 * 21) == 3              # all three alternatives of one position
    assert {140 + 105 * 24} <= {r["pos"] - 1 for r in loose} and 140 + 105 * 23 not in {r["pos"] - 1 for r in loose}   # alternative depth 3 / 2
    no_bal = pileup_cases.reference(by["filters_no_balance"])[0]
    assert [r["sor"] for r in no_bal if r["pos"] - 1 == 140 + 105 * 20] == [-1.0]
    no_end = {(r["seq_id"], r["pos"] - 1) for r in pileup_cases.reference(by["filters_no_end"])[0]}
    assert {(0, L[0] - K), (1, K - 1), (4, K), (5, K - 1), (6, 7)} <= no_end
