#!/usr/bin/env python3
"""One SARS-CoV-2 sample of 1 M reads of 150 bases, a share of them reads across a jump on one strand -- backward (the junction of a
tandem duplication at a random cell, of a random length) or forward (the same jump as a deletion) --, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/duplications_profile.py SHARE backward|forward [reads]
`backward` enables duplications (where the library has them) next to junctions and gives the time of duplication_scan_kernel;
`forward` enables junctions alone and gives junction_scan_kernel's time on the same reads with the jumps turned round, which is the
yardstick: the same anchors, the same span work, as many walks of the same lengths."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

SHARE = float(sys.argv[1]) if len(sys.argv) > 1 else 0.001
BACKWARD = (sys.argv[2] if len(sys.argv) > 2 else "backward") == "backward"
N_READS = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
LEN = 150

ref = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
g = synth.read_fasta_bytes(ref)
codes = synth.CODE[np.frombuffer(bytes(g), np.uint8)]
L = len(codes)
rng = np.random.default_rng(17)
starts = rng.integers(0, L - LEN, N_READS)
reads = codes[starts[:, None] + np.arange(LEN)[None, :]].astype(np.uint8)
jump = np.flatnonzero(rng.random(N_READS) < SHARE)
if len(jump):                                        # `left` bases that end at cell x - 1, the rest from cell y on
    n = len(jump)
    left = rng.integers(40, LEN - 40, n)[:, None]
    dist = rng.integers(33, 3000, n)[:, None]
    x = rng.integers(3200, L - 3200, n)[:, None]
    y = x - dist if BACKWARD else x + dist
    j = np.arange(LEN)[None, :]
    reads[jump] = codes[np.where(j < left, x - left + j, y + j - left)]
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

ix = HostIndex.build(21, [ref])
eng = ix.engine()
eng.junctions_enable(33, 2, 20)
duplications = BACKWARD and hasattr(eng, "duplications_enable")
if duplications:
    eng.duplications_enable(33, 2, 20)
for rep in range(3):
    eng.sample_begin()
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_junctions(1)
    jsum = eng.download_junctions(cap=0)[0]
    if duplications:
        eng.sample_duplications(1)
        dsum = eng.download_duplications(cap=0)[0]
print("share %g %s: %d records; junctions: %d anchored, %d reference-spanning, %d supporting, %d backward, %d discordant, %d events" %
      (SHARE, "backward" if BACKWARD else "forward", jsum.records, jsum.anchored, jsum.ref_spanning, jsum.supporting, jsum.backward, jsum.discordant, jsum.candidates))
if duplications:
    print("duplications: %d anchored, %d reference-spanning, %d supporting, %d short, %d forward, %d discordant, %d events" %
          (dsum.anchored, dsum.ref_spanning, dsum.supporting, dsum.short_, dsum.forward, dsum.discordant, dsum.candidates))
eng.close()
ix.close()
