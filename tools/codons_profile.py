#!/usr/bin/env python3
"""One SARS-CoV-2 sample of 1 M reads of 150 bases with linkage enabled, then bk_sample_linkage at 40 sites and bk_sample_codons over
the three whole-genome frames, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/codons_profile.py random|amplicon [reads]
which gives the times of codon_count_lds_kernel / codon_count_kernel and codon_finish_kernel next to link_count_kernel's on the same
rows.  `random`: every read starts anywhere; `amplicon`: every read starts at one of 100 cells.  The three
frames (29.9 k codons) take the device-memory path of the cover array; the first frame alone (10 k) the LDS path: both are run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "random"
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
LEN = 150

ref = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
g = synth.read_fasta_bytes(ref)
codes = synth.CODE[np.frombuffer(bytes(g), np.uint8)]
L = len(codes)
rng = np.random.default_rng(11)
hap = codes.copy()                                   # a haplotype of 40 substitutions carried by 60 % of the reads
sites = np.sort(rng.choice(np.arange(300, L - 300), 40, replace=False))
hap[sites] = (hap[sites] + 1) % 4
if MODE == "amplicon":
    starts = rng.choice(np.arange(0, L - LEN, (L - LEN) // 100)[:100], N_READS)
else:
    starts = rng.integers(0, L - LEN, N_READS)
at = starts[:, None] + np.arange(LEN)[None, :]
reads = np.where((rng.random(N_READS) < 0.6)[:, None], hap[at], codes[at]).astype(np.uint8)
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

ix = HostIndex.build(21, [ref])
eng = ix.engine()
eng.linkage_enable(8, N_READS)
frames = [(f, (L - f) // 3) for f in range(3)]
eng.sample_begin()
eng.push_reads(0, words, lens)
eng.sample_finalize(1)
for rep in range(3):
    eng.sample_linkage([int(s) for s in sites], 1000)
    lsum, _ = eng.download_linkage()
    eng.sample_codons(frames)
    csum, counts = eng.download_codons()
    eng.sample_codons(frames[:1])
    csum1, counts1 = eng.download_codons()
    assert np.array_equal(counts[:len(counts1)], counts1)
print("%s: %d records, %d placed, %d pairs, %d codons in %d regions, largest cover %d, counts that are not the largest of their codon %d" %
      (MODE, lsum.records, csum.rows, lsum.n_pairs, csum.n_codons, csum.n_regions, int(counts.sum(axis=1).max()),
       int(counts.sum() - counts.max(axis=1).sum())))
eng.close()
ix.close()
