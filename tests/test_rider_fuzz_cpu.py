"""The random cases of tests/rider_fuzz.py without a GPU: the host twins (hostlib.indel_events, link_rows, link_count, codon_count,
hap_count, read_pileup_count) against the Python restatements, over the very iterations that tests/test_gpu_rider_fuzz.py runs on the
engine -- every indel event with its forward and reverse counts, the whole prefix-summed span array, the five counters, the rows, the
tallies, every pair, codon and haplotype, the twelve read-pileup counters of every cell at two end distances.  The trimmed iterations
(adapters and primers set) give the twins the reads as tests/adapter_ref.py and primer_ref.py leave them.  Then the conditions that
keep the fuzz from being vacuous, asserted on the restatements' results alone and summed over those iterations."""
import functools

import numpy as np
import pytest

from tests import rider_fuzz


@functools.lru_cache(maxsize=None)
def _case(it, trim=False):
    case = rider_fuzz.make_case(rider_fuzz.SEED, it, trim)
    return case, (rider_fuzz.expected(case) if case is not None else None)


def _host_block(block, trim):
    bad = []
    for it in range(block * rider_fuzz.BLOCK, (block + 1) * rider_fuzz.BLOCK):
        case, exp = _case(it, trim)
        if case is None:
            continue
        try:
            rider_fuzz.check_host(case, exp)
        except AssertionError as e:
            bad.append("%s: %s" % (case.describe(), str(e)[:400]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("block", range(rider_fuzz.BLOCKS))
def test_host_twins_equal_the_restatements(block):
    _host_block(block, False)


@pytest.mark.parametrize("block", range(rider_fuzz.TRIM_BLOCKS))
def test_host_twins_equal_the_restatements_of_trimmed_reads(block):
    _host_block(block, True)


def _second(case):
    return (case.pile_end, case.pile_at, case.pile_row, case.pile_d, case.recheck)


def _trimming(case):
    return (case.trim, case.adapters, case.min_overlap, case.max_error_rate, case.primers, case.primer_m)


def test_a_case_is_a_function_of_seed_and_iteration():
    a, b = rider_fuzz.make_case(7, 3), rider_fuzz.make_case(7, 3)
    assert a.describe() == b.describe() and a.reads == b.reads and a.seqs == b.seqs and a.sites == b.sites and a.hap_regions == b.hap_regions
    assert rider_fuzz.make_case(7, 4).reads != a.reads and rider_fuzz.make_case(8, 3).reads != a.reads
    # the second generator's fields
    assert _second(a) == _second(b) and _trimming(a) == (False, [], 5, 0.1, [], 1)
    assert len({_second(rider_fuzz.make_case(7, it)) for it in range(8)}) == 8
    assert a.pile_end in (0, 1, 10, a.k, 80, 128, 255) and a.pile_at in (0, 1, 2) and a.pile_d in (-1, 0, 1) and 0 <= a.pile_row < 1
    ea, eb = rider_fuzz.expected(a), rider_fuzz.expected(b)
    assert ea.ends == eb.ends and ea.ends[0] == a.pile_end and all(np.array_equal(ea.pile[E], eb.pile[E]) for E in ea.ends)
    assert ea.ends[1] in {min(255, (r[1] + a.pile_d) // 2) for r in ea.rows}


def test_a_trimmed_case_is_the_same_base_case_and_a_function_of_seed_and_iteration():
    a, t, u = rider_fuzz.make_case(7, 3), rider_fuzz.make_case(7, 3, True), rider_fuzz.make_case(7, 3, True)
    assert _trimming(t) == _trimming(u) and t.reads == u.reads and t.quals == u.quals and t.describe() == u.describe() and t.trim
    assert rider_fuzz.make_case(7, 4, True).primers != t.primers
    # the base case: the genome, every parameter, the second generator's first draws, and the reads that were not rewritten
    assert (t.seqs, t.k, t.sites, t.codon_regions, t.hap_regions, t.push, t.batch, t.n_mates) == (a.seqs, a.k, a.sites, a.codon_regions, a.hap_regions, a.push, a.batch, a.n_mates)
    assert _second(t) == _second(a) and len(t.reads) == len(a.reads)
    same = sum(x == y for x, y in zip(t.reads, a.reads))
    assert 0 < same < len(a.reads) and all(len(r) == len(q) for r, q in zip(t.reads, t.quals))
    # only what bk_adapters_set and bk_primers_set accept
    src = "".join(t.seqs)
    assert 1 <= len(t.adapters) <= 3 and all(12 <= len(x) <= 30 and set(x) <= set(b"ACGT") for x in t.adapters)
    assert t.min_overlap in (3, 5, 12) and t.min_overlap <= min(len(x) for x in t.adapters) and t.max_error_rate in (0.0, 0.1, 0.2)
    assert 1 <= len(t.primers) <= 6 and t.primer_m in (0, 1, 2)
    for p in t.primers:
        assert 18 <= len(p) <= 30 and (p.decode() in src or rider_fuzz.indels_ref.revcomp(p.decode()) in src)


def test_the_fuzz_is_not_vacuous():
    t = {}
    for it in range(rider_fuzz.BLOCKS * rider_fuzz.BLOCK):
        case, exp = _case(it)
        if case is not None:
            rider_fuzz.tally(case, exp, t)
    print(sorted(t.items()))
    floors = dict(placed=2000, placed_fwd=500, placed_rev=500, discordant=1000, unplaced=2000, rows_8_mismatches=20, events=100, deletions=30, insertions=30,
                  max_len_turned_away=10, it_several_sequences=15, it_n_run=15, it_rc_repeat=15, it_global_pairs=15, it_record_over_300=15)
    # the read pileup, at about half of what the restatements give for the suite's seed: rows that are near an end at every cell (n <= 2E) and
    # rows with two stretches, rows at n = 2E - 1, 2E and 2E + 1, substitutions near an end and not, near-end counts, the cases at the
    # smallest and the largest end distance, each place of the count among the others, genomes of fewer cells than the finish kernel has
    # threads, and chunks of 64 rows with more groups of equal (strand, first cell) than a wave has merge rounds
    floors.update(pile_rows_whole=3000, pile_rows_split=3900, pile_rows_at_2e=370, pile_subs_near=2900, pile_subs_far=1500, pile_near_counts=550000,
                  it_pile_end_0=8, it_pile_end_255=10, it_pile_at_0=18, it_pile_at_1=20, it_pile_at_2=20, it_under_1024_cells=5,
                  pile_waves=88, pile_waves_over_4_groups=3)
    floors.update({"k=%d" % k: 5 for k in set(rider_fuzz.KS)})
    short = {name: (t.get(name, 0), floor) for name, floor in floors.items() if t.get(name, 0) < floor}
    assert not short, short
    # what the specification says must occur at all: sequences shorter than k and than 2k, an N run at a sequence's first or last cell
    assert t["it_seq_under_k"] >= 1 and t["it_seq_under_2k"] >= 1 and t["it_n_run_at_an_end"] >= 1, t
    assert t["codon_counts"] > 0 and t["hap_entries"] > 0 and t["pair_counts"] > 0, t


def test_the_trimmed_fuzz_is_not_vacuous():
    """The trimmed blocks, on the restatements' results alone: the adapters cut, the primers mask at either end, reads are emptied or
    left shorter than k, and what is left still feeds every pass behind the scan -- each floor at about half of the suite's seed's."""
    t = {}
    for it in range(rider_fuzz.TRIM_BLOCKS * rider_fuzz.BLOCK):
        case, exp = _case(it, True)
        if case is not None:
            rider_fuzz.tally(case, exp, t)
    print(sorted(t.items()))
    floors = dict(trim_reads_cut=1000, trim_bases_removed=85000, trim_5=650, trim_3=270, trim_bases_masked=22000, trim_reads_emptied=250,
                  placed=1750, placed_fwd=850, placed_rev=900, events=95, deletions=55, insertions=35, codon_counts=35000, hap_entries=80, pair_counts=55000,
                  pile_rows_whole=1600, pile_rows_split=1950, pile_rows_at_2e=110, pile_subs_near=1400, pile_subs_far=900, pile_waves_over_4_groups=10,
                  it_under_1024_cells=3, it_pile_end_0=5, it_pile_end_255=5)
    short = {name: (t.get(name, 0), floor) for name, floor in floors.items() if t.get(name, 0) < floor}
    assert not short, short
