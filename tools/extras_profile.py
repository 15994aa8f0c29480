#!/usr/bin/env python3
"""Two samples with every optional pass on (full_kmer_stats, k-mer dump, indels, linkage, primers, an adapter, calls, consensus,
regions) over tests/golden/hpv.bkdb: the workload for `rocprofv3 --kernel-trace --stats -- python tools/extras_profile.py [reads]`,
which gives the riding kernels' times (kmer_dump_count_kernel, indel_scan_kernel, link_scan_kernel, link_count_kernel).
BRONKO_HIP_LIB selects another build of the library, as for tools/ab.sh."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import Params, synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_READS = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
BATCHES = 4

ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
g = synth.read_fasta_bytes(os.path.join(GOLDEN, "HPV16.fa"))
gm, isnv = synth.sample_genome(g, 1)
reads = synth.codes_to_ascii(synth.single_end_codes(gm, N_READS, 150, 1, isnv=isnv))
eng = ix.engine(Params(full_kmer_stats=True, kmer_table_log2=22))
eng.adapters_set([b"AGATCGGAAGAGC"], 5, 0.1)
eng.primers_set([bytes(g[p:p + 22]) for p in range(1720, 3700, 97)], 1)
eng.kmer_dump_enable(24)
eng.indels_enable()
eng.linkage_enable(8, 2 * N_READS)
eng.regions_set([(0, 0, s, s + 400) for s in range(0, 7600, 400)])
sites = list(range(100, 7800, 50))
per = (N_READS + BATCHES - 1) // BATCHES
for sample in range(2):
    eng.sample_begin()
    for b in range(BATCHES):
        eng.push_reads_ascii(0, reads[b * per:(b + 1) * per])
    res = eng.sample_finish(1)
    eng.sample_call(1, eng.call_params(min_depth=10))
    eng.sample_consensus()
    eng.sample_region_depths(10)
    eng.sample_indels(1, 0)
    eng.sample_linkage(sites, 1000)
    isum, _ = eng.download_indels()
    lsum, _ = eng.download_linkage()
    print("sample %d: %d records, %d anchored (indels), %d placed (linkage), %d pairs, %d k-mers kept" %
          (sample, isum.records, isum.anchored, lsum.placed, lsum.n_pairs, eng.kmer_dump_size(0)[0]))
eng.close()
ix.close()
