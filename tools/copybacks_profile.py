#!/usr/bin/env python3
"""One SARS-CoV-2 sample of 1 M reads of 150 bases, a share of them strand switches (copy-backs of both kinds at random pairs of
cells), with junctions and -- where the library has them -- copy-backs enabled, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/copybacks_profile.py SHARE [reads]
which gives the time of copyback_scan_kernel next to junction_scan_kernel's on the same records.  The
junction pass does the same anchor and span work and walks none of these records; that is the yardstick."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

SHARE = float(sys.argv[1]) if len(sys.argv) > 1 else 0.001
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
LEN = 150

ref = os.path.join(ROOT, "tests", "golden", "4_sarscov2", "wuhan_ref.fasta")
g = synth.read_fasta_bytes(ref)
codes = synth.CODE[np.frombuffer(bytes(g), np.uint8)]
L = len(codes)
rng = np.random.default_rng(13)
starts = rng.integers(0, L - LEN, N_READS)
reads = codes[starts[:, None] + np.arange(LEN)[None, :]].astype(np.uint8)
turn = np.flatnonzero(rng.random(N_READS) < SHARE)
if len(turn):                                        # arm A: la bases that end at cell x; arm B: the rest, from cell y on, on the other strand
    n = len(turn)
    la = rng.integers(40, LEN - 40, n)[:, None]
    x, y = (rng.integers(LEN, L - LEN, n)[:, None] for _ in range(2))
    kind_t = (rng.random(n) < 0.5)[:, None]
    j = np.arange(LEN)[None, :]
    in_a = j < la
    cell = np.where(kind_t, np.where(in_a, x + la - 1 - j, y + j - la), np.where(in_a, x - la + 1 + j, y - (j - la)))
    down = np.where(kind_t, in_a, ~in_a)             # this arm runs down the reference: it reads the complement
    reads[turn] = np.where(down, 3 - codes[cell], codes[cell])
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

ix = HostIndex.build(21, [ref])
eng = ix.engine()
eng.junctions_enable()
copybacks = hasattr(eng, "copybacks_enable")
if copybacks:
    eng.copybacks_enable(2, 20)
for rep in range(3):
    eng.sample_begin()
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_junctions(1)
    jsum = eng.download_junctions(cap=0)[0]
    if copybacks:
        eng.sample_copybacks(1)
        csum = eng.download_copybacks(cap=0)[0]
print("share %g: %d records; junctions: %d anchored, %d reference-spanning" % (SHARE, jsum.records, jsum.anchored, jsum.ref_spanning))
if copybacks:
    print("copy-backs: %d on one strand, %d reference-spanning, %d switched, %d supporting, %d discordant, %d events" %
          (csum.same_strand, csum.ref_spanning, csum.switched, csum.supporting, csum.discordant, csum.candidates))
eng.close()
ix.close()
