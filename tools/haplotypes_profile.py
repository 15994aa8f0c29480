#!/usr/bin/env python3
"""One SARS-CoV-2 sample of 1 M reads of 150 bases with linkage enabled, then bk_sample_haplotypes over windows of 100 every 50 cells
and bk_sample_codons over the first whole-genome frame, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/haplotypes_profile.py random|amplicon [reads]
which gives the times of hap_count_kernel and hap_finish_kernel next to codon_count_lds_kernel's on the same rows (DESIGN.md section
H).  `random`: every read starts anywhere; `amplicon`: every read starts at one of 100 cells.  A haplotype of 40 substitutions is
carried by 30 % of the reads: on the amplicon input its lists are single counters that thousands of rows add to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import BronkoError, synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "random"
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
LEN, WINDOW, STEP = 150, 100, 50

ref = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
g = synth.read_fasta_bytes(ref)
codes = synth.CODE[np.frombuffer(bytes(g), np.uint8)]
L = len(codes)
rng = np.random.default_rng(11)
hap = codes.copy()                                   # a haplotype of 40 substitutions carried by 30 % of the reads
sites = np.sort(rng.choice(np.arange(300, L - 300), 40, replace=False))
hap[sites] = (hap[sites] + 1) % 4
if MODE == "amplicon":
    starts = rng.choice(np.arange(0, L - LEN, (L - LEN) // 100)[:100], N_READS)
else:
    starts = rng.integers(0, L - LEN, N_READS)
at = starts[:, None] + np.arange(LEN)[None, :]
reads = np.where((rng.random(N_READS) < 0.3)[:, None], hap[at], codes[at]).astype(np.uint8)
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

ix = HostIndex.build(21, [ref])
eng = ix.engine()
eng.linkage_enable(8, N_READS)
windows = [(s, WINDOW) for s in range(0, L - WINDOW + 1, STEP)]
eng.sample_begin()
eng.push_reads(0, words, lens)
eng.sample_finalize(1)
log2 = 20
for rep in range(3):
    while True:
        eng.sample_haplotypes(windows, log2)
        try:
            hsum, cover, ref_count, entries = eng.download_haplotypes(cap=0 if rep else None)
            break
        except BronkoError as e:                     # the table was full: four times the slots
            if e.status != -6 or log2 >= 24:
                raise
            print("table_log2 %d: %d counts dropped" % (log2, e.hap[0].dropped))
            log2 += 2
    eng.sample_codons([(0, L // 3)])
    csum, counts = eng.download_codons()
    if rep == 0:
        top = max(n for _, n, _ in entries)
        assert all(int(cover[r]) >= n for r, n, _ in entries) and int(cover.sum()) == int(ref_count.sum()) + sum(n for _, n, _ in entries)
print("%s: %d placed, %d regions, %d without cover, %d distinct non-reference haplotypes in a table of 2^%d slots, largest count %d, largest cover %d; %d codons" %
      (MODE, hsum.rows, hsum.n_regions, int((cover == 0).sum()), hsum.entries, hsum.table_log2, top, int(cover.max()), csum.n_codons))
eng.close()
ix.close()
