"""--adapter on the host (no GPU): the Python restatement of the contract (tests/adapter_ref.py) against itself -- numpy against
letter by letter --, the host packer on the truncated reads against its record-level counts, what `bronko call` refuses before it
touches a device, the presets, the new symbols of the C ABI, and that the generated reads exercise what the GPU tests rely on."""
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import _ffi, pack_reads_ends, synth

from tests import adapter_ref, primer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TRUSEQ, NEXTERA = adapter_ref.PRESETS["truseq"], adapter_ref.PRESETS["nextera"]
LONG_ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"   # 33 bases: three 16-base words


@pytest.fixture(scope="module")
def bronko():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bronko_amd", "host"), "../bin/bronko"])
    return BRONKO


def dataset(genome, seed, adapters, O=5, E=0.1, n=1500, read_len=150):
    """(reads, tags, amplicons, primers): library reads of a sample of the genome at 150 bases (some at 32 and 300) and the edge cases"""
    gm, _ = synth.sample_genome(genome, seed)
    amps = primer_ref.tile_amplicons(genome, seed)
    primers = [p for a in amps for p in a[2:]]
    reads = adapter_ref.library_reads(gm, amps, adapters, n, read_len, seed + 1)
    tags = ["library"] * len(reads)
    for rl, s in ((32, 2), (300, 3)):
        extra = adapter_ref.library_reads(gm, amps, adapters, n // 8, rl, seed + s)
        reads += extra
        tags += ["library %d" % rl] * len(extra)
    for r, t in adapter_ref.edge_reads(genome, adapters, O, E, read_len, seed + 4):
        reads.append(r)
        tags.append(t)
    return reads, tags, amps, primers


def quals_for(reads, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        qv = rng.integers(30, 41, len(r))
        qv[rng.random(len(r)) < 0.01] = 7
        if len(r) > 40 and i % 17 == 1:
            qv[-9] = 3           # inside the adapter or the tail: only what lies behind it is searched
        out.append((qv + 33).astype(np.uint8).tobytes())
    return out


@pytest.fixture(scope="module")
def hpv():
    return synth.read_fasta_bytes(os.path.join(GOLDEN, "HPV16.fa"))


@pytest.mark.parametrize("adapters,O,E", [([TRUSEQ], 5, 0.1), ([LONG_ADAPTER, NEXTERA, TRUSEQ], 3, 0.1), ([NEXTERA, b"ACGTTGCA"], 8, 0.3),
                                          ([LONG_ADAPTER], 5, 0.0)])
def test_numpy_reference_equals_letter_by_letter(hpv, adapters, O, E):
    reads, tags, _, _ = dataset(hpv, 5, adapters, O, E, n=500)
    reads += [r for r, _ in adapter_ref.long_reads(hpv, adapters, 6)[2:4]] + [b"", b"N", b"ACG", b"NNNN" + adapters[0]]
    quals = quals_for(reads, 7)
    for min_qual in (0, 20):
        cuts, s1 = adapter_ref.cut_positions_all(reads, adapters, O, E, quals, min_qual)
        for i, r in enumerate(reads):
            if len(r) <= 400 or i % 2:
                assert int(cuts[i]) == adapter_ref.cut_position(r, adapters, O, E, quals[i], min_qual), (i, r[:200])
        assert (cuts >= 0).sum() > 100


def test_reference_by_hand():
    A = TRUSEQ
    f = lambda r, O=5, E=0.1, ad=(A,): adapter_ref.cut_position(r, list(ad), O, E)
    body = b"ACCATGGTTACAGGCATTACCGATTAGCCA"
    assert f(body + A + b"TTTT") == 30                       # the whole adapter inside the read
    assert f(body + A[:5]) == 30 and f(body + A[:4]) == -1   # a prefix of O bases at the end; one base fewer is none
    assert f(A + body) == 0                                  # a dimer
    assert f(body + b"AGATCGGTAGAGC" + b"TT") == 30          # 13 bases, floor(1.3) = 1 mismatch
    assert f(body + b"AGATCGGTAGTGC" + b"TT") == -1          # two
    assert f(body + b"AGATCGGTAG") == 30                     # 10 bases at the end: floor(1.0) = 1
    assert f(body + b"AGATCGGTA") == -1                      # 9 bases: floor(0.9) = 0
    assert f(body + A + b"N" + body) == -1                   # only the last run of valid letters is searched
    assert f(body + b"N" + body[:7] + A.lower()) == 38       # ... from its start; case folded
    assert f(body + A + body + A) == 30                      # the leftmost match
    assert adapter_ref.cut_position(body + A, [A], 5, 0.1, b"I" * 30 + b"#" + b"I" * 12, 20) == -1   # a masked base inside the adapter
    assert adapter_ref.cut_position(body + A, [A], 5, 0.1, b"I" * 30 + b"#" + b"I" * 12, 0) == 30
    assert adapter_ref.truncate([b"ACGT", b"ACGT", b"ACGT"], [b"IIII"] * 3, [-1, 0, 2]) == ([b"ACGT", b"N", b"AC"], [b"IIII", b"!", b"II"])
    assert adapter_ref.allowed(0.1, 10) == 1 and adapter_ref.allowed(0.1, 30) == 3 and adapter_ref.allowed(0.3, 64) == 19


def unpack(words, lens):
    return [bytes(b"ACGT"[(int(w[i >> 4]) >> (2 * (i & 15))) & 3] for i in range(int(l))) for w, l in zip(words, lens)]


@pytest.mark.parametrize("adapters", [[TRUSEQ], [LONG_ADAPTER, NEXTERA, TRUSEQ]])
def test_host_packer_on_truncated_reads_agrees_with_the_record_counts(hpv, adapters):
    """The records the host packer makes of the raw and of the truncated reads, with their end flags: the bases in records that end
    their read fall by exactly what bk_adapter_stats is defined to report (plus what is left of the emptied records), and no
    other record changes."""
    k = 21
    reads, _, _, _ = dataset(hpv, 9, adapters, n=800)
    quals = [b"I" * len(r) for r in reads]
    cuts, s1 = adapter_ref.cut_positions_all(reads, adapters, 5, 0.1)
    trunc, _ = adapter_ref.truncate(reads, quals, cuts)
    n_cut, removed = adapter_ref.record_counts(reads, cuts, s1, k)
    n_empty, empty_bases = adapter_ref.emptied(reads, cuts, s1, k)
    assert n_cut > 200 and n_empty > 0
    w0, l0, e0 = pack_reads_ends(reads, k)
    w1, l1, e1 = pack_reads_ends(trunc, k)
    assert unpack(w1, l1) == [b for b, _ in primer_ref.end_flags(trunc, k)] and e1.tolist() == [f for _, f in primer_ref.end_flags(trunc, k)]
    last0, last1 = (e0 & 2) != 0, (e1 & 2) != 0
    assert int(l0[last0].sum()) - int(l1[last1].sum()) == removed + empty_bases
    assert len(l0) - len(l1) == n_empty
    assert sorted(unpack(w0[~last0], l0[~last0])) == sorted(unpack(w1[~last1], l1[~last1]))


def test_generated_reads_exercise_the_feature(hpv):
    """Asserted on the Python reference, so that a GPU test cannot pass while nothing is cut."""
    adapters, O, E, k = [LONG_ADAPTER, NEXTERA, TRUSEQ], 5, 0.1, 21
    reads, tags, amps, primers = dataset(hpv, 40, adapters, O, E)
    long = adapter_ref.long_reads(hpv, adapters, 41)
    reads += [r for r, _ in long]
    tags += [t for _, t in long]
    assert {32, 150, 300} <= {len(r) for r in reads}
    cuts, s1 = adapter_ref.cut_positions_all(reads, adapters, O, E)
    assert (cuts >= 0).mean() >= 0.30, (cuts >= 0).mean()
    n = np.array([len(r) for r in reads])
    assert ((cuts >= 0) & (n - cuts < 10) & (n - cuts >= O)).sum() >= 1                        # a partial match under 10 bases
    part = {}                                                                                # every partial length O .. LA is cut
    for i, t in enumerate(tags):
        if t.startswith("partial "):
            l = int(t.split()[1])
            part.setdefault(l, []).append(i)
            assert l < O or 0 <= cuts[i] <= len(reads[i]) - l, (l, reads[i])
    assert set(part) == set(range(O - 1, max(len(A) for A in adapters) + 1))
    assert any(cuts[i] < 0 for i in part[O - 1])                                             # ... and O - 1 is too short an overlap
    assert ((cuts == 0) & (s1 == 0) & (n > 0)).sum() >= 3                                      # dimers
    exact = sum(1 for i in np.flatnonzero(cuts >= 0) if any(d == a > 0 for d, a in adapter_ref.hamming_at_cut(reads[i], cuts[i], s1[i], adapters, E)))
    assert exact >= 1                                                                        # a match at exactly the allowance
    assert sum(1 for i, t in enumerate(tags) if t == "near miss" and cuts[i] < 0) >= 1         # one mismatch more: left as it is
    assert sum(1 for i, t in enumerate(tags) if t == "at the allowance" and cuts[i] >= 0) >= 1
    assert sum(1 for i, t in enumerate(tags) if t == "deep" and len(reads[i]) >= 20000 and cuts[i] >= 15000) >= 1
    assert all(cuts[i] < 0 for i, t in enumerate(tags) if t == "too long")
    hidden = [i for i, t in enumerate(tags) if t == "before an N"]                           # (what lies behind the N may match by chance)
    assert all(cuts[i] < 0 or cuts[i] > reads[i].rindex(b"N") for i in hidden) and sum(1 for i in hidden if cuts[i] < 0) >= 2
    assert any(len(r) > adapter_ref.MAXB for r, t in zip(reads, tags) if t == "too long")
    assert any(t == "N inside" for t in tags) and any(t == "lower case" and cuts[i] >= 0 for i, t in enumerate(tags))
    # a read whose 3' primer is found only after the cut
    trunc, _ = adapter_ref.truncate(reads, [b"I" * len(r) for r in reads], cuts)
    late = sum(1 for i in np.flatnonzero(cuts > 0)[:3000] if len(reads[i]) <= 400
               and primer_ref.trim_lengths(reads[i], primers, 1)[1] == 0 and primer_ref.trim_lengths(trunc[i], primers, 1)[1] > 0)
    assert late >= 10, late
    # ... and the counters are not trivially equal to the read-level ones
    assert adapter_ref.record_counts(reads, cuts, s1, k)[0] < (cuts >= 0).sum()


# ---- bronko call --adapter: what is refused before any device is touched ----------------------------------------------------------
def call_with(bronko, tmp_path, extra):
    fq = str(tmp_path / "r.fastq")
    open(fq, "wb").write(b"".join(b"@r%d\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" % i for i in range(4)))
    return subprocess.run([bronko, "call", "-d", os.path.join(GOLDEN, "hpv.bkdb"), "-r", fq, "-o", str(tmp_path / "o")] + extra,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case,extra,needle", [
    ("symbol", ["--adapter", "truseq", "AGATCGGAAGNGC"], ["adapter 2", "'N'", "ACGT"]),
    ("unknown preset", ["--adapter", "trueseq"], ["adapter 1", "truseq", "nextera"]),
    ("length 7", ["--adapter", "AGATCGG"], ["adapter 1", "7 bases", "between 8 and 64"]),
    ("length 65", ["--adapter", "nextera", "ACGT" * 16 + "A"], ["adapter 2", "65 bases", "between 8 and 64"]),
    ("9 adapters", ["--adapter"] + ["AGATCGGAAGAGC"] * 9, ["9 adapters", "at most 8"]),
    ("overlap 2", ["--adapter", "truseq", "--adapter-min-overlap", "2"], ["between 3 and", "got 2"]),
    ("overlap -1", ["--adapter", "truseq", "--adapter-min-overlap=-1"], ["between 3 and", "got -1"]),
    ("overlap above the shortest", ["--adapter", "nextera", "ACGTACGTAC", "--adapter-min-overlap", "11"], ["between 3 and", "(10)", "got 11"]),
    ("rate -0.1", ["--adapter", "truseq", "--adapter-error-rate", "-0.1"], ["between 0 and 0.3", "got -0.1"]),
    ("rate 0.31", ["--adapter", "truseq", "--adapter-error-rate", "0.31"], ["between 0 and 0.3", "got 0.31"]),
    ("rate nan", ["--adapter", "truseq", "--adapter-error-rate", "nan"], ["between 0 and 0.3"]),
    ("overlap without adapter", ["--adapter-min-overlap", "5"], ["--adapter-min-overlap needs --adapter"]),
    ("rate without adapter", ["--adapter-error-rate", "0.1"], ["--adapter-error-rate needs --adapter"]),
])
def test_cli_refuses_bad_adapters(bronko, tmp_path, case, extra, needle):
    res = call_with(bronko, tmp_path, extra)
    assert res.returncode == 1, (res.stdout, res.stderr)
    for s in needle:
        assert s in res.stdout + res.stderr, (s, res.stdout, res.stderr)
    assert not os.path.exists(str(tmp_path / "o"))   # (refused before anything is made)


def test_cli_presets_expand(bronko, tmp_path):
    """--debug names the adapters as check_call_args expanded them (the run itself needs a device: its exit code is not looked at)"""
    res = call_with(bronko, tmp_path, ["--adapter", "truseq", "nextera", "acgtacgtac", "--adapter-min-overlap", "10", "--adapter-error-rate", "0.3",
                                       "--debug"])
    log = res.stdout + res.stderr
    assert "adapter 1: AGATCGGAAGAGC" in log and "adapter 2: CTGTCTCTTATACACATCT" in log and "adapter 3: acgtacgtac" in log, log
    assert adapter_ref.PRESETS == {"truseq": b"AGATCGGAAGAGC", "nextera": b"CTGTCTCTTATACACATCT"}


def test_cli_usage_names_the_options(bronko):
    res = subprocess.run([bronko, "--help"], capture_output=True, text=True, timeout=60)
    for s in ("--adapter SEQ", "--adapter-min-overlap", "--adapter-error-rate", "truseq", "nextera"):
        assert s in res.stdout + res.stderr, s


def test_library_exports_the_adapter_symbols():
    hdr = open(os.path.join(ROOT, "include", "bronko_hip.h")).read()
    for testing in (False, True):
        L = _ffi.load(testing=testing)
        for s in ("bk_adapters_set", "bk_adapter_stats"):
            assert hasattr(L, s) and s in _ffi.SYMBOLS and s + "(" in hdr, s
        assert L.bk_abi_version() == 8
