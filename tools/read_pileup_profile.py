#!/usr/bin/env python3
"""One SARS-CoV-2 sample of 1 M reads of 150 bases with linkage enabled, then bk_sample_read_pileup, bk_sample_codons over the first
whole-genome frame and bk_sample_haplotypes over windows of 100 every 50 cells, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/read_pileup_profile.py shotgun|amplicon [reads]
which gives the times of read_pileup_count_kernel and read_pileup_finish_kernel next to codon_count_lds_kernel's and hap_count_kernel's
on the same rows.  `shotgun`: every read starts anywhere; `amplicon`: every read starts at one cell, so that
every row adds to the same words of the difference arrays.  A haplotype of 40 substitutions is carried by 30 % of the reads: on the
amplicon input each of its substitutions under the amplicon is one counter that 300,000 rows add to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "shotgun"
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
LEN, WINDOW, STEP, END = 150, 100, 50, 10

ref = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
g = synth.read_fasta_bytes(ref)
codes = synth.CODE[np.frombuffer(bytes(g), np.uint8)]
L = len(codes)
rng = np.random.default_rng(11)
hap = codes.copy()                                   # a haplotype of 40 substitutions carried by 30 % of the reads
sites = np.sort(rng.choice(np.arange(300, L - 300), 40, replace=False))
AMPLICON = int(sites[20]) - 70                       # the one amplicon lies over a site of the haplotype
hap[sites] = (hap[sites] + 1) % 4
starts = np.full(N_READS, AMPLICON) if MODE == "amplicon" else rng.integers(0, L - LEN, N_READS)
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
for rep in range(3):
    eng.sample_read_pileup(END)
    psum, cells = eng.download_read_pileup(cap=None if rep == 0 else 0)
    eng.sample_codons([(0, L // 3)])
    csum, counts = eng.download_codons()
    eng.sample_haplotypes(windows, 20)
    hsum = eng.download_haplotypes(cap=0)[0]
    if rep == 0:
        depth = cells[:, :8].astype(np.int64).sum(axis=1)
        assert int(depth.sum()) == psum.bases == psum.rows * LEN and int((depth > 0).sum()) == psum.covered
        top, top_mm = int(depth.max()), int(np.sort(cells[:, :8].astype(np.int64), axis=1)[:, -2].max())
print("%s: %d placed, %d of %d positions covered, %d bases, largest depth %d, largest count of a second base %d; %d codons, %d haplotype regions" %
      (MODE, psum.rows, psum.covered, psum.n_cells, psum.bases, top, top_mm, csum.n_codons, hsum.n_regions))
eng.close()
ix.close()
