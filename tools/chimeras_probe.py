#!/usr/bin/env python3
"""One sample of 1 M reads of 150 bases of a genome of eight sequences (random letters, 900 to 2,400 each: the shape of an
influenza index), a share of them junctions between two sequences in all four orientations at random pairs of cells, with
copy-backs and chimeras enabled on one engine, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/chimeras_probe.py [SHARE [reads]]
which gives the time of chimera_scan_kernel next to copyback_scan_kernel's on the same records.  The
copy-back pass does the same anchor and span work and walks none of these records; that is the yardstick."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bronko_amd import synth  # noqa: E402
from bronko_amd.hostlib import HostIndex  # noqa: E402

SHARE = float(sys.argv[1]) if len(sys.argv) > 1 else 0.01
N_READS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
LEN = 150

rng = np.random.default_rng(17)
lengths = [2341, 2341, 2233, 1778, 1565, 1413, 1027, 890]
seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lengths]
codes = np.concatenate(seqs)
first = np.concatenate([[0], np.cumsum(lengths)])
seg = rng.integers(0, 8, N_READS)
starts = first[seg] + (rng.random(N_READS) * (np.array(lengths)[seg] - LEN)).astype(np.int64)
reads = codes[starts[:, None] + np.arange(LEN)[None, :]].astype(np.uint8)
cross = np.flatnonzero(rng.random(N_READS) < SHARE)
if len(cross):                                       # arm A: la bases that end at cell x of one sequence; arm B: the rest, from cell y of another
    n = len(cross)
    la = rng.integers(40, LEN - 40, n)[:, None]
    sx = rng.integers(0, 8, n)
    sy = (sx + rng.integers(1, 8, n)) % 8
    x = (first[sx] + LEN + (rng.random(n) * (np.array(lengths)[sx] - 2 * LEN)).astype(np.int64))[:, None]
    y = (first[sy] + LEN + (rng.random(n) * (np.array(lengths)[sy] - 2 * LEN)).astype(np.int64))[:, None]
    a_down, b_down = (rng.random(n) < 0.5)[:, None], (rng.random(n) < 0.5)[:, None]
    j = np.arange(LEN)[None, :]
    in_a = j < la
    cell = np.where(in_a, np.where(a_down, x + la - 1 - j, x - la + 1 + j), np.where(b_down, y - (j - la), y + j - la))
    down = np.where(in_a, a_down, b_down)            # this arm runs down the reference: it reads the complement
    reads[cross] = np.where(down, 3 - codes[cell], codes[cell])
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

letters = np.frombuffer(b"ACGT", np.uint8)
ix = HostIndex.build_mem(21, [("segments", [("seg%d" % (i + 1), letters[s].tobytes()) for i, s in enumerate(seqs)])])
eng = ix.engine()
eng.copybacks_enable(2, 20)
eng.chimeras_enable(2, 20)
for rep in range(3):
    eng.sample_begin()
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_copybacks(1)
    csum = eng.download_copybacks(cap=0)[0]
    eng.sample_chimeras(1)
    xsum = eng.download_chimeras(cap=0)[0]
print("share %g: %d records; copy-backs: %d on one strand, %d reference-spanning, %d switched" % (SHARE, csum.records, csum.same_strand, csum.ref_spanning, csum.switched))
print("chimeras: %d on one strand of one sequence, %d reference-spanning, %d crossed, %d supporting, %d discordant, %d events" %
      (xsum.same_strand, xsum.ref_spanning, xsum.crossed, xsum.supporting, xsum.discordant, xsum.candidates))
eng.close()
ix.close()
