"""Kernel times of --adapter: 1 M x 150 bp reads of SARS-CoV-2, about 45 % of them read through into an adapter (30 % short
shotgun inserts and the short amplicons),
device-resident sequence lines; per round one sample plain, one with PROBE_ADAPTERS (1 or 3, default 1) adapters set, and one with
the adapters and the primers of a tiling of the genome.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/adapters_probe.py` and read adapter_find_kernel, adapter_trim_kernel,
primer_trim_kernel, pack_words_ends_kernel, pack_words_kernel and scan_items_kernel off the kernel statistics; without the profiler
it prints wall times per sample."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bronko_amd import Params, synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402
from tests import adapter_ref, primer_ref  # noqa: E402

ADAPTERS = [b"AGATCGGAAGAGC", b"CTGTCTCTTATACACATCT", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"]


def main():
    n_unique, tile, rounds = 100000, 10, int(os.environ.get("PROBE_ROUNDS", "4"))
    adapters = ADAPTERS[:int(os.environ.get("PROBE_ADAPTERS", "1"))]
    fa = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
    g = synth.read_fasta_bytes(fa)
    ix = HostIndex.build(21, [fa])
    eng = ix.engine(Params(device=0))
    gm, _ = synth.sample_genome(g, 1)
    amps = primer_ref.tile_amplicons(g, 1)
    primers = [p for a in amps for p in a[2:]]
    reads = adapter_ref.library_reads(gm, amps, adapters, n_unique, 150, 2, short=0.3, amplicon=0.4)
    cuts, _ = adapter_ref.cut_positions_all(reads[:20000], adapters, 5, 0.1)
    print("adapters %d, primers %d, reads %d x %d, cut: %.3f" % (len(adapters), len(primers), n_unique, tile, (cuts >= 0).mean()))
    flat = np.frombuffer(b"".join(reads) * tile, np.uint8)
    n = n_unique * tile
    off = np.arange(n + 1, dtype=np.int64) * 150
    d_b = torch.from_numpy(flat.copy()).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    torch.cuda.synchronize()
    for r in range(rounds + 1):   # (round 0 warms up)
        for what in ("plain", "adapters", "adapters + primers"):
            eng.adapters_set(adapters if what != "plain" else [], 5, 0.1)
            eng.primers_set(primers if what == "adapters + primers" else [], 1)
            t0 = time.perf_counter()
            eng.sample_begin()
            eng.push_reads_ascii_device(0, d_b.data_ptr(), d_off.data_ptr(), n, n * 150, 150)
            res = eng.sample_finish(1)
            dt = time.perf_counter() - t0
            if r:
                print("round %d %s: %.3f ms a sample (push to downloaded result), k-mers %d%s" % (
                    r, what, dt * 1e3, int(res.kmer_stats[0][1]), ", stats %s" % eng.adapter_stats(0) if what != "plain" else ""))
    eng.close()


if __name__ == "__main__":
    main()
