"""bk_sample_consensus (consensus_kernel) against the Python restatement (tests/consensus_ref.py): on crafted pileups the way
tests/test_gpu_calls_crafted.py gets them onto the device -- a sample of selection reads is finalized, the device pileup is
overwritten, bk_sample_call selects the genome, then the consensus is made of what is there --, the call order and parameter checks
of the C ABI, and `bronko call --consensus` end to end on reads with planted substitutions and a stretch nothing covers."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bronko_amd import BronkoError, synth
from tests import consensus_ref, helpers, pileup_cases

pytestmark = pytest.mark.gpu
K = pileup_cases.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")


def _to_call(eng, case):
    """The case's pileup on the device and bk_sample_call run on it."""
    import torch
    from bronko_amd import pack_reads
    from bronko_amd.dist import DeviceVector
    eng.sample_begin()
    words, lens = pack_reads(case.layout.selection_reads(), K)
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_download(1, arrays=False)                         # (synchronises: the finalize has written its pileup)
    cells4 = eng.total_cells * 4
    assert cells4 == len(case.fwd)
    dev = torch.as_tensor(DeviceVector(eng.pileup_ptr(), 4 * cells4), device="cuda:0")
    dev.copy_(torch.from_numpy(np.concatenate(case.arrays()).view(np.int64)))
    torch.cuda.synchronize()
    eng.sample_call(1, case.params.apply(eng.call_params()))


def _check(eng, case):
    """Letters and tallies of the case at each of its parameter pairs; returns the number of letters compared."""
    _to_call(eng, case)
    n = 0
    for d, f in consensus_ref.params_of(case):
        want_letters, want = consensus_ref.expected(case, d, f)
        eng.sample_consensus(eng.consensus_params(min_depth=d, min_freq=f))
        summ, letters = eng.download_consensus()
        assert summ.file_id == case.layout.target, case.name
        got = {name: getattr(summ, name) for name in consensus_ref.TALLIES}
        assert got == want, (case.name, d, f)
        if letters != want_letters:
            bad = [i for i in range(len(want_letters)) if letters[i:i + 1] != want_letters[i:i + 1]]
            raise AssertionError("%s at D = %d, F = %r: %d letters differ, first at %d: %r, expected %r" %
                                 (case.name, d, f, len(bad), bad[0], letters[bad[0]:bad[0] + 1], want_letters[bad[0]:bad[0] + 1]))
        n += len(letters)
    return n


class _Engines:
    """An engine per layout, made inside the test."""

    def __init__(self, oracle):
        self.oracle, self.by_layout = oracle, {}

    def get(self, lay):
        if lay.name not in self.by_layout:
            ix = self.oracle.Index.build_mem(K, lay.files)
            self.by_layout[lay.name] = (ix, helpers.engine_from_oracle_index(ix))
        return self.by_layout[lay.name][1]

    def close(self):
        for ix, eng in self.by_layout.values():
            eng.close()
            ix.close()


def _run_all(oracle, cases):
    engines, n = _Engines(oracle), 0
    try:
        for case in cases:
            n += _check(engines.get(case.layout), case)
    finally:
        engines.close()
    return n


def test_crafted_cases(oracle):
    cases = consensus_ref.crafted_cases()
    assert {c.layout.name for c in cases} == {"lengths", "multi", "filters", "tie"}
    assert _run_all(oracle, cases) > 4 * 10000


def test_random_mix(oracle):
    assert _run_all(oracle, consensus_ref.random_cases()) > 200 * 4 * 700


def test_two_samples_in_a_row_and_on_a_fork(oracle):
    """A pileup that covers every sequence of the long genome, then one of the short genome of the same files, then a sparse one of the
    long genome again, on one engine -- letters and tallies of the sample before must not show --, the same on a fork of that engine,
    and once more on the engine itself."""
    by = {c.name: c for c in consensus_ref.named_cases()}
    heavy, sparse = by["table_increasing"], by["lengths_sparse"]
    short = [c for c in consensus_ref.crafted_cases() if c.name == "consensus_short_genome"][0]   # the other genome of the same files
    assert heavy.layout is sparse.layout and short.layout.files is heavy.layout.files
    assert sum(n for _, n in short.layout.seqs) == 150 < sum(n for _, n in heavy.layout.seqs)
    ix = oracle.Index.build_mem(K, heavy.layout.files)
    eng = helpers.engine_from_oracle_index(ix)
    fork = eng.fork()
    try:
        for e in (eng, fork, eng):
            _check(e, heavy)
            _check(e, short)
            _check(e, sparse)
    finally:
        fork.close()
        eng.close()
        ix.close()


def test_selection_tie_takes_the_lowest_id(oracle):
    case = pileup_cases.tie_case()
    ix = oracle.Index.build_mem(K, case.layout.files)
    eng = helpers.engine_from_oracle_index(ix)
    try:
        _check(eng, case)
        summ, _ = eng.download_consensus()
        assert summ.file_id == 0
    finally:
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
        from bronko_amd import pack_reads
        assert status(eng.sample_consensus)[0] == -5             # BK_ERR_STATE: nothing was ever called
        eng.sample_begin()
        assert status(eng.sample_consensus)[0] == -5             # inside a sample
        words, lens = pack_reads(lay.selection_reads(), K)
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        assert status(eng.sample_consensus)[0] == -5             # finalized, but not called
        assert status(eng.download_consensus)[0] == -5
        _to_call(eng, case)
        st, msg = status(eng.sample_consensus, eng.consensus_params(min_depth=0))
        assert st == -1 and "min_depth" in msg                  # BK_ERR_INVALID, the parameter named
        st, msg = status(eng.sample_consensus, eng.consensus_params(min_freq=1.5))
        assert st == -1 and "min_freq" in msg
        assert status(eng.sample_consensus, eng.consensus_params(min_freq=float("nan")))[0] == -1
        eng.sample_consensus()
        want_letters, want = consensus_ref.expected(case, 10, 0.5)
        summ, letters = eng.download_consensus(cap=100)          # fewer than the genome has: `cap` letters, the full count
        assert summ.positions == want["positions"] == len(want_letters) > 100 and letters == want_letters[:100]
        import ctypes as C
        from bronko_amd import _ffi
        raw, rs = np.full(200, 0xff, np.uint8), _ffi.ConsensusSummary()   # ... and nothing behind them is written
        assert eng._L.bk_sample_download_consensus(eng.h, C.byref(rs), raw.ctypes.data_as(C.c_void_p), 100) == 0
        assert raw[:100].tobytes() == want_letters[:100] and (raw[100:] == 0xff).all() and rs.positions == len(want_letters)
        summ, letters = eng.download_consensus(cap=len(want_letters) + 50)
        assert letters == want_letters
        eng.sample_begin()                                       # the next sample: the selection is no longer this sample's
        assert status(eng.sample_consensus)[0] == -5
        assert status(eng.download_consensus)[0] == -5
        eng.push_reads(0, words, lens)
        eng.sample_finalize(1)
        assert status(eng.sample_consensus)[0] == -5             # ... not before its own bk_sample_call
        eng.sample_call(1)
        eng.sample_consensus()
        assert eng.download_consensus()[0].file_id == lay.target
    finally:
        eng.close()
        ix.close()


def test_no_genome_selected(oracle):
    """A sample without reads selects nothing: file_id -1, every tally 0, no letters."""
    lay = pileup_cases.layout("multi")
    ix = oracle.Index.build_mem(K, lay.files)
    eng = helpers.engine_from_oracle_index(ix)
    try:
        eng.sample_begin()
        eng.sample_finalize(1)
        eng.sample_call(1)
        eng.sample_consensus()
        summ, letters = eng.download_consensus()
        assert summ.file_id == -1 and letters == b""
        assert [getattr(summ, name) for name in consensus_ref.TALLIES] == [0, 0, 0, 0, 0]
    finally:
        eng.close()
        ix.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
GAP = (3000, 3600)                                               # no read covers these positions of HPV16


def _sample(golden_dir, paired):
    g = synth.read_fasta_bytes(os.path.join(golden_dir, "HPV16.fa"))
    gm, isnv = synth.sample_genome(g, 31, n_snp=8, n_isnv=4)
    planted = [(i, gm[i]) for i in range(len(g)) if gm[i] != g[i] and not GAP[0] - 200 <= i < GAP[1] + 200 and 200 <= i < len(g) - 200]
    assert len(planted) >= 2
    mates = [[], []]
    for part, (lo, hi) in enumerate(((0, GAP[0]), (GAP[1], len(g)))):   # reads of either side of the gap: none reaches into it
        piece = gm[lo:hi]
        shifted = [(p - lo, alt, af) for p, alt, af in isnv if lo <= p < hi]
        n = 4000 * (hi - lo) // len(g)
        if paired:
            c1, c2 = synth.paired_codes(piece, n // 2, 150, 310 + part, isnv=shifted)
            mates[0] += synth.codes_to_ascii(c1)
            mates[1] += synth.codes_to_ascii(c2)
        else:
            mates[0] += synth.codes_to_ascii(synth.single_end_codes(piece, n, 150, 310 + part, isnv=shifted))
    return g, planted, mates[:2 if paired else 1]


@pytest.mark.parametrize("inflate", ["one", "many"])
@pytest.mark.parametrize("paired", [False, True])
def test_cli_consensus_end_to_end(oracle, golden_dir, tmp_path, paired, inflate):
    g, planted, mates = _sample(golden_dir, paired)
    paths = []
    for m, reads in enumerate(mates):
        p = str(tmp_path / ("cons_R%d.fastq.gz" % (m + 1)))
        with gzip.open(p, "wb", compresslevel=1) as f:
            for i, r in enumerate(reads):
                f.write(b"@r%d_%d\n%s\n+\n%s\n" % (m, i, r, b"I" * len(r)))
        paths.append(p)
    db = os.path.join(golden_dir, "hpv.bkdb")
    reads_args = ["-1", paths[0], "-2", paths[1]] if paired else ["-r", paths[0]]
    env = dict(os.environ, BRONKO_INFLATE_THREADS="1") if inflate == "one" else dict(os.environ)
    outs = {}
    for name, extra in (("with", ["--consensus"]), ("without", [])):
        out = str(tmp_path / name)
        res = subprocess.run([BRONKO, "call", "-d", db] + reads_args + ["--pileup", "-o", out, "-t", "8"] + extra,
                             capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        assert ("inflated on" in res.stdout + res.stderr) == (inflate == "many")
        assert ("Consensus of" in res.stdout) == (name == "with")
        outs[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    stem = "cons_R1"
    assert set(outs["with"]) == set(outs["without"]) | {stem + ".consensus.fa"}
    assert set(outs["without"]) == {stem + ".vcf", stem + ".tsv", "bronko_overview.tsv"}
    for f in outs["without"]:                                    # the VCF, the pileup TSV and the overview do not know of the flag
        assert outs["with"][f] == outs["without"][f], f
    # the writer's format over the restatement applied to the oracle's pileup of the same reads
    ix = oracle.Index.load(db)
    try:
        pile = oracle.sample_pileup(ix, mates)
        assert oracle.pick_best_genome(ix, pile.stats.sum(axis=0), pile.present.max(axis=0)) == 0
        files = ix.files()
        seqs, at = [], 0
        for _, s in files[0][1]:
            seqs.append((at, len(s)))
            at += len(s)
        ref_codes = np.array([pileup_cases._CODE.get(c, 0) for _, s in files[0][1] for c in s], np.uint8)
        letters, tallies = consensus_ref.consensus(seqs, ref_codes, pile.fwd_depth, pile.rev_depth, 10, 0.5)
        names = [name.split()[0] for name, _ in files[0][1]]
        got = outs["with"][stem + ".consensus.fa"]
        assert got == consensus_ref.fasta_text(stem, names, seqs, letters)
    finally:
        ix.close()
    text = b"".join(got.split(b"\n")[1:])
    assert len(text) == len(g)
    for pos, base in planted:                                    # the planted bases, and the gap as a run of N
        assert text[pos] == base != g[pos], pos
    assert text[GAP[0]:GAP[1]] == b"N" * (GAP[1] - GAP[0]) and tallies["masked"] >= GAP[1] - GAP[0]
    assert tallies["substitutions"] >= len(planted)
