"""The random cases of tests/rider_fuzz.py without a GPU: the host twins (hostlib.indel_events, link_rows, link_count, codon_count,
hap_count) against the Python restatements, over the very iterations that tests/test_gpu_rider_fuzz.py runs on the engine -- every
indel event with its forward and reverse counts, the whole prefix-summed span array, the five counters, the rows, the tallies, every
pair, codon and haplotype.  Then the conditions that keep the fuzz from being vacuous, asserted on the restatements' results alone and
summed over those iterations."""
import functools

import pytest

from tests import rider_fuzz


@functools.lru_cache(maxsize=None)
def _case(it):
    case = rider_fuzz.make_case(rider_fuzz.SEED, it)
    return case, (rider_fuzz.expected(case) if case is not None else None)


@pytest.mark.parametrize("block", range(rider_fuzz.BLOCKS))
def test_host_twins_equal_the_restatements(block):
    bad = []
    for it in range(block * rider_fuzz.BLOCK, (block + 1) * rider_fuzz.BLOCK):
        case, exp = _case(it)
        if case is None:
            continue
        try:
            rider_fuzz.check_host(case, exp)
        except AssertionError as e:
            bad.append("%s: %s" % (case.describe(), str(e)[:400]))
    assert not bad, "\n".join(bad)


def test_a_case_is_a_function_of_seed_and_iteration():
    a, b = rider_fuzz.make_case(7, 3), rider_fuzz.make_case(7, 3)
    assert a.describe() == b.describe() and a.reads == b.reads and a.seqs == b.seqs and a.sites == b.sites and a.hap_regions == b.hap_regions
    assert rider_fuzz.make_case(7, 4).reads != a.reads and rider_fuzz.make_case(8, 3).reads != a.reads


def test_the_fuzz_is_not_vacuous():
    t = {}
    for it in range(rider_fuzz.BLOCKS * rider_fuzz.BLOCK):
        case, exp = _case(it)
        if case is not None:
            rider_fuzz.tally(case, exp, t)
    print(sorted(t.items()))
    floors = dict(placed=2000, placed_fwd=500, placed_rev=500, discordant=1000, unplaced=2000, rows_8_mismatches=20, events=100, deletions=30, insertions=30,
                  max_len_turned_away=10, it_several_sequences=15, it_n_run=15, it_rc_repeat=15, it_global_pairs=15, it_record_over_300=15)
    floors.update({"k=%d" % k: 5 for k in set(rider_fuzz.KS)})
    short = {name: (t.get(name, 0), floor) for name, floor in floors.items() if t.get(name, 0) < floor}
    assert not short, short
    # what the specification says must occur at all: sequences shorter than k and than 2k, an N run at a sequence's first or last cell
    assert t["it_seq_under_k"] >= 1 and t["it_seq_under_2k"] >= 1 and t["it_n_run_at_an_end"] >= 1, t
    assert t["codon_counts"] > 0 and t["hap_entries"] > 0 and t["pair_counts"] > 0, t
