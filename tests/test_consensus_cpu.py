"""`bronko call --consensus` without a GPU: the host twin of consensus_kernel (caller.cpp consensus) against the Python restatement
(tests/consensus_ref.py) on the crafted pileups, the pileups of tests/pileup_cases.py and its random mix; the FASTA writer byte for
byte; the argument checks of the binary."""
import os
import subprocess

import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex
from tests import consensus_ref, pileup_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
K = pileup_cases.K


def _check_cases(cases):
    by_layout, n = {}, 0
    try:
        for case in cases:
            lay = case.layout
            if lay.name not in by_layout:
                by_layout[lay.name] = HostIndex.build_mem(K, lay.files)
            ix = by_layout[lay.name]
            for d, f in consensus_ref.params_of(case):
                want_letters, want = consensus_ref.expected(case, d, f)
                letters, tallies = hostlib.consensus(ix, lay.target, case.fwd, case.rev, d, f)
                got = dict(zip(consensus_ref.TALLIES, tallies))
                assert got == want, (case.name, d, f)
                if letters != want_letters:
                    bad = [i for i in range(len(letters)) if letters[i] != want_letters[i]]
                    raise AssertionError("%s at D = %d, F = %r: %d letters differ, first at %d: %c, expected %c" %
                                         (case.name, d, f, len(bad), bad[0], letters[bad[0]], want_letters[bad[0]]))
                assert len(letters) == sum(length for _, length in lay.seqs)
                n += 1
    finally:
        for ix in by_layout.values():
            ix.close()
    return n


def test_host_twin_on_the_crafted_cases():
    assert _check_cases(consensus_ref.crafted_cases()) >= 4 * len(consensus_ref.crafted_cases())


def test_host_twin_on_the_named_pileups():
    _check_cases(consensus_ref.named_cases())


def test_host_twin_on_the_random_mix():
    assert _check_cases(consensus_ref.random_cases()) == 200 * len(consensus_ref.PARAMS)


def test_the_crafted_cases_reach_every_set_and_both_sides_of_the_depth_rule():
    sets, masked, unmasked = consensus_ref.coverage_of(consensus_ref.crafted_cases())
    assert sets == set(range(1, 16)) and masked and unmasked
    # what the cases are there for, stated on the restatement itself
    bs = consensus_ref.base_set
    assert bs((9, 0, 0, 0), 10, 0.5) is None and bs((10, 0, 0, 0), 10, 0.5) == 1 and bs((0, 0, 11, 0), 10, 0.5) == 4
    assert bs((50, 50, 0, 0), 1, 0.5) == 3 and bs((50, 30, 20, 0), 1, 0.5) == 1 and bs((49, 31, 20, 0), 1, 0.5) == 3
    assert bs((40, 30, 30, 0), 1, 0.5) == 7 and bs((25, 25, 25, 25), 1, 0.5) == 15
    assert bs((30, 10, 5, 0), 1, 0.0) == 1 and bs((30, 30, 10, 0), 1, 0.0) == 3 and bs((5, 3, 1, 0), 1, 1.0) == 7
    assert bs((1, 1, 1, 0), 1, 1.0 / 3.0) == 7 and bs((2, 1, 0, 0), 1, 0.7) == 3 and bs((3, 2, 2, 0), 1, 0.7) == 7 and bs((4, 3, 0, 0), 1, 0.7) == 3
    assert consensus_ref.LETTERS[15] == "N" and consensus_ref.LETTERS[5] == "R"
    # a substitution is counted against the reference code, a non-ACGT letter as A
    case = [c for c in consensus_ref.crafted_cases() if c.name == "consensus_ref_letters_0"][0]
    other = [c for c in consensus_ref.crafted_cases() if c.name == "consensus_ref_letters_1"][0]
    assert consensus_ref.expected(case, 10, 0.5)[1]["substitutions"] == 0 and consensus_ref.expected(other, 10, 0.5)[1]["substitutions"] == 6
    lay = case.layout
    assert consensus_ref.expected(case, 10, 0.5)[0][140 + 105 * 4] == ord("A") and lay.files[1][1][0][1][140 + 105 * 4] == ord("N")


@pytest.mark.parametrize("lengths", [[1], [60], [61], [1100], [1, 60, 61, 1100]])
def test_writer_byte_for_byte(tmp_path, lengths):
    import random
    rng = random.Random(sum(lengths))
    seqs = [("seq%d some description" % j, pileup_cases.random_sequence(rng, n)) for j, n in enumerate(lengths)]
    files = [("other", [("o1", pileup_cases.random_sequence(rng, 30))]), ("genome", seqs)]
    ix = HostIndex.build_mem(K, files)
    try:
        letters = bytes(rng.choice(b"ACGTNRYKM-") for _ in range(sum(lengths)))
        path = str(tmp_path / "x.consensus.fa")
        hostlib.write_consensus_fasta(path, "sample_1", ix, 1, letters)
        cells, at = [], 0
        for n in lengths:
            cells.append((at, n))
            at += n
        want = consensus_ref.fasta_text("sample_1", ["seq%d" % j for j in range(len(lengths))], cells, letters)
        got = open(path, "rb").read()
        assert got == want
        if lengths == [61]:
            assert got == b">sample_1|seq0\n" + letters[:60] + b"\n" + letters[60:] + b"\n"
        with pytest.raises(RuntimeError):                     # letters that are not the genome's length
            hostlib.write_consensus_fasta(path, "sample_1", ix, 1, letters + b"A")
    finally:
        ix.close()


def test_cli_refuses_bad_consensus_arguments(golden_dir, tmp_path):
    db = os.path.join(golden_dir, "hpv.bkdb")
    fq = str(tmp_path / "x.fastq")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    for extra, word in ((["--consensus", "--consensus-min-depth", "0"], "depth"),
                        (["--consensus", "--consensus-min-freq", "1.5"], "frequency"),
                        (["--consensus", "--consensus-min-freq", "-0.1"], "frequency"),
                        (["--consensus-min-depth", "5"], "--consensus"),
                        (["--consensus-min-freq", "0.6"], "--consensus")):
        r = subprocess.run([BRONKO, "call", "-d", db, "-r", fq, "-o", str(tmp_path / "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stdout and word in r.stdout, (extra, r.stdout, r.stderr)
        assert "no HIP device" not in r.stdout                # refused before any device is touched
    usage = subprocess.run([BRONKO, "--help"], capture_output=True, text=True).stderr
    for opt in ("--consensus", "--consensus-min-depth", "--consensus-min-freq"):
        assert opt in usage
