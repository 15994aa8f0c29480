"""The ingest buffers under reuse (bk_ingest.cpp): one mate file pushed as batches whose sizes go small, large, small, so that every
ASCII slot (three, in rotation), both packed staging slots and the device pushes' shared buffers (bk_engine::dev_ascii) are used
again after their first batch and have to grow then -- with adapters and primers set, so the end-flag buffers and the adapters'
per-record scratch grow with them.  Each push path on its own, and the two device paths that share dev_ascii in alternation.  Every
run equals, bit for bit, the same reads pushed as one batch, the oracle on the trimmed reads, and the reference counters."""
import os

import numpy as np
import pytest

from bronko_amd import pack_reads_ends, synth

from tests import adapter_ref, helpers, primer_ref
from tests.adapter_ref import seen_reads as expected
from tests.test_gpu_adapters import TRUSEQ, quals_for

pytestmark = pytest.mark.gpu

K, O, E, M, MIN_QUAL = 21, 5, 0.1, 1, 20
SIZES = [64, 32, 64, 2048, 1024, 4096, 64, 32]   # reads of 150 bases per batch


def grows_after_first_use(sizes, n_slots):
    """every slot of a rotation of n_slots meets, after its first batch, one four times as large: more than its slack holds (a
    quarter, and for the sequence lines of these batches at most as much again)"""
    return all(any(s >= 4 * sizes[slot] for s in sizes[slot + n_slots::n_slots]) for slot in range(n_slots))


class World:
    def __init__(self, oracle):
        import torch
        self.ix = oracle.Index.load(os.path.join(helpers.GOLDEN, "hpv.bkdb"))
        g = synth.read_fasta_bytes(os.path.join(helpers.GOLDEN, "HPV16.fa"))
        gm, _ = synth.sample_genome(g, 7)
        amps = primer_ref.tile_amplicons(g, 7)
        self.adapters, self.primers = [TRUSEQ], [p for a in amps for p in a[2:]]
        self.reads = adapter_ref.library_reads(gm, amps, self.adapters, sum(SIZES), 150, 8)
        self.quals = quals_for(self.reads, 9)
        self.cut = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
        # what every run must give, per quality threshold: the oracle on the trimmed reads and the reference counters
        self.want = {}
        for mq in (0, MIN_QUAL):
            trimmed, counts, pcounts, _ = expected(self.reads, self.quals, self.adapters, O, E, K, mq, self.primers, M)
            assert counts[0] > 100 and pcounts[0] > 100 and pcounts[1] > 100
            self.want[mq] = (oracle.sample_pileup(self.ix, [trimmed]), counts, pcounts)
        flat, qflat = np.frombuffer(b"".join(self.reads), np.uint8), np.frombuffer(b"".join(self.quals), np.uint8)
        self.off = np.zeros(len(self.reads) + 1, np.int64)
        self.off[1:] = np.cumsum([len(r) for r in self.reads])
        pad = np.zeros(64, np.uint8)   # (the packer stages whole 16-byte units)
        self.d_b = torch.from_numpy(np.concatenate([flat, pad])).to("cuda:0")
        self.d_q = torch.from_numpy(np.concatenate([qflat, pad])).to("cuda:0")
        self.keep = []   # device arrays of a run: alive until its finalize has been waited for

    def engine(self):
        """a fresh engine (its buffers have held nothing yet) with the adapters and the primers set"""
        eng = helpers.engine_from_oracle_index(self.ix)
        eng.adapters_set(self.adapters, O, E)
        eng.primers_set(self.primers, M)
        return eng

    def on_device(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        torch.cuda.synchronize()
        self.keep.append(t)
        return t

    # the push paths: reads [a, b) of the mate file as one call
    def ascii_qual(self, eng, a, b):
        eng.push_reads_ascii(0, self.reads[a:b], self.quals[a:b], MIN_QUAL)

    def packed_ends(self, eng, a, b):
        w, l, e = pack_reads_ends(self.reads[a:b], K)
        eng.push_reads_ends(0, w, l, e)

    def packed_ends_device(self, eng, a, b):
        w, l, e = pack_reads_ends(self.reads[a:b], K)
        d_w, d_l, d_e = self.on_device(w.view(np.int32)), self.on_device(l.view(np.int16)), self.on_device(e)
        eng.push_reads_ends_device(0, d_w.data_ptr(), w.shape[1], d_l.data_ptr(), d_e.data_ptr(), len(l))

    def ascii_device(self, eng, a, b, min_qual=0):
        d_off = self.on_device(self.off[a:b + 1] - self.off[a])
        at = int(self.off[a])   # (150-base reads: the batches start at every alignment mod 16)
        eng.push_reads_ascii_device(0, self.d_b.data_ptr() + at, d_off.data_ptr(), b - a, int(self.off[b] - self.off[a]), 150,
                                    quals=self.d_q.data_ptr() + at if min_qual else None, min_qual=min_qual)

    def ascii_qual_device(self, eng, a, b):
        self.ascii_device(eng, a, b, MIN_QUAL)

    def run(self, eng, pushes):
        """one sample from (path, a, b) pushes -> (result, adapter counters, primer counters)"""
        eng.sample_begin()
        for path, a, b in pushes:
            path(eng, a, b)
        res = eng.sample_finish(1)
        self.keep.clear()
        return res, eng.adapter_stats(0), eng.primer_stats(0)


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.ix.close()


def test_the_batches_make_every_slot_grow_after_its_first_use():
    assert len(SIZES) >= 7 and grows_after_first_use(SIZES, 3) and grows_after_first_use(SIZES, 2) and grows_after_first_use(SIZES, 1)


@pytest.mark.parametrize("paths,min_qual", [
    (("ascii_qual",), MIN_QUAL), (("packed_ends",), 0), (("packed_ends_device",), 0), (("ascii_qual_device",), MIN_QUAL),
    (("ascii_device", "packed_ends_device"), 0)], ids=lambda v: "+".join(v) if isinstance(v, tuple) else None)
def test_batches_that_reuse_and_grow_the_buffers_equal_one_batch(world, paths, min_qual):
    paths = [getattr(world, p) for p in paths]
    pile, counts, pcounts = world.want[min_qual]
    eng = world.engine()
    # (the batches first: the one batch leaves its buffers large enough for every batch behind it)
    split = world.run(eng, [(paths[i % len(paths)], a, b) for i, (a, b) in enumerate(zip(world.cut, world.cut[1:]))])
    whole = world.run(eng, [(paths[-1], 0, len(world.reads))])
    eng.close()
    for res, ac, pc in (whole, split):
        helpers.assert_same_pileup(res, pile)
        assert ac == counts and pc == pcounts
    assert np.array_equal(split[0].kmer_stats, whole[0].kmer_stats)
    for name in ("fwd_depth", "rev_depth", "fwd_nk", "rev_nk", "stats", "present"):
        assert np.array_equal(getattr(split[0], name), getattr(whole[0], name)), name
