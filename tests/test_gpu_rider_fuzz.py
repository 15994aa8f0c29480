"""The random cases of tests/rider_fuzz.py on the engine: indel_scan_kernel, link_scan_kernel, link_count_kernel, the codon, the
haplotype and the read-pileup kernels against the Python restatements, one engine per iteration (create, enable, sample, every
download, close).  The read pileup is counted twice per sample, once among the other counts and once behind them, at an end distance
of a fixed list and at one that is half a row's length.  The trimmed blocks set adapters and primers first (adapter_find_kernel,
adapter_trim_kernel, the primer kernels in front of every pass) and assert their counters per mate.  Every comparison is exact.  tests/test_rider_fuzz_cpu.py runs the same iterations through the host twins and asserts what they exercise;
tools/fuzz_riders.py reproduces a failing iteration from the line a mismatch prints."""
import pytest

from tests import rider_fuzz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("block", range(rider_fuzz.BLOCKS))
def test_engine_equals_the_restatements(block):
    ran, bad = rider_fuzz.run(rider_fuzz.SEED, block * rider_fuzz.BLOCK, rider_fuzz.BLOCK, rider_fuzz.check_engine)
    assert ran > 0 and not bad, "\n".join("%s: %s" % b for b in bad)


@pytest.mark.parametrize("block", range(rider_fuzz.TRIM_BLOCKS))
def test_engine_equals_the_restatements_of_trimmed_reads(block):
    ran, bad = rider_fuzz.run(rider_fuzz.SEED, block * rider_fuzz.BLOCK, rider_fuzz.BLOCK, rider_fuzz.check_engine, trim=True)
    assert ran > 0 and not bad, "\n".join("%s: %s" % b for b in bad)
