"""Kernel times of --primers: 1 M x 150 bp amplicon reads of SARS-CoV-2 with the primers of a tiling of the
genome, device-resident sequence lines, one sample with primers set and one without, alternating.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/primers_probe.py` and read primer_trim_kernel, pack_words_ends_kernel,
pack_words_kernel and scan_items_kernel off the kernel statistics; without the profiler it prints wall times per sample."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bronko_amd import Params, synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402
from tests import primer_ref  # noqa: E402


def main():
    n_unique, tile, rounds = 100000, 10, int(os.environ.get("PROBE_ROUNDS", "4"))
    fa = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
    g = synth.read_fasta_bytes(fa)
    ix = HostIndex.build(21, [fa])
    eng = ix.engine(Params(device=0))
    gm, _ = synth.sample_genome(g, 1)
    amps = primer_ref.tile_amplicons(g, 1)
    primers = [p for a in amps for p in a[2:]]
    reads = [r.ljust(150, b"A")[:150] for r in primer_ref.amplicon_reads(g, gm, amps, n_unique, 150, 2, shotgun=0.0)]
    p5, p3, _, _ = primer_ref.trim_lengths_all(reads, primers, 1)
    print("primers %d, reads %d x %d, p5 > 0: %.3f, p3 > 0: %.3f" % (len(primers), n_unique, tile, (p5 > 0).mean(), (p3 > 0).mean()))
    flat = np.frombuffer(b"".join(reads) * tile, np.uint8)
    n = n_unique * tile
    off = np.arange(n + 1, dtype=np.int64) * 150
    d_b = torch.from_numpy(flat.copy()).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    for r in range(rounds + 1):   # (round 0 warms up)
        for with_primers in (False, True):
            eng.primers_set(primers if with_primers else [], 1)
            t0 = time.perf_counter()
            eng.sample_begin()
            eng.push_reads_ascii_device(0, d_b.data_ptr(), d_off.data_ptr(), n, n * 150, 150)
            res = eng.sample_finish(1)
            dt = time.perf_counter() - t0
            if r:
                print("round %d primers %d: %.3f ms a sample (push to downloaded result), k-mers %d%s" % (
                    r, with_primers, dt * 1e3, int(res.kmer_stats[0][1]), ", stats %s" % eng.primer_stats(0) if with_primers else ""))
    eng.close()


if __name__ == "__main__":
    main()
