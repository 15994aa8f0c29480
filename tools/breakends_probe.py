#!/usr/bin/env python3
"""One sample of 1 M reads of 150 bases of a genome of eight sequences (random letters, 900 to 2,400 each: the shape of an
influenza index), a share of them clipped -- their last 30 to 90 bases replaced by random ones, at one of 200 sites or anywhere --,
with junctions and breakends enabled on one engine, three times: the workload for
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/breakends_probe.py [SHARE [reads]]
which gives the time of breakend_scan_kernel next to junction_scan_kernel's on the same records.  The
junction pass does the same anchor lookups and the same Hamming pass and walks none of these records; that is the yardstick."""
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

rng = np.random.default_rng(19)
lengths = [2341, 2341, 2233, 1778, 1565, 1413, 1027, 890]
seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lengths]
codes = np.concatenate(seqs)
first = np.concatenate([[0], np.cumsum(lengths)])
seg = rng.integers(0, 8, N_READS)
starts = first[seg] + (rng.random(N_READS) * (np.array(lengths)[seg] - LEN)).astype(np.int64)
clip = np.flatnonzero(rng.random(N_READS) < SHARE)
if len(clip):                                        # half of the clipped reads end their held part at one of 200 sites
    sites = rng.integers(0, len(codes) - 2 * LEN, 200) + LEN
    at = rng.random(len(clip)) < 0.5
    held = rng.integers(LEN - 90, LEN - 30 + 1, len(clip))
    site = sites[rng.integers(0, 200, len(clip))]
    starts[clip] = np.where(at, site - held + 1, starts[clip])
reads = codes[np.clip(starts[:, None] + np.arange(LEN)[None, :], 0, len(codes) - 1)].astype(np.uint8)
if len(clip):
    tail = np.arange(LEN)[None, :] >= held[:, None]
    reads[clip] = np.where(tail, rng.integers(0, 4, (len(clip), LEN)).astype(np.uint8), reads[clip])
err = rng.random(reads.shape) < 0.005
reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
back = rng.random(N_READS) < 0.5                     # half of the reads against the reference
reads[back] = 3 - reads[back][:, ::-1]
words, lens = synth.pack_codes(reads)

letters = np.frombuffer(b"ACGT", np.uint8)
ix = HostIndex.build_mem(21, [("segments", [("seg%d" % (i + 1), letters[s].tobytes()) for i, s in enumerate(seqs)])])
eng = ix.engine()
eng.junctions_enable(33, 2, 20)
eng.breakends_enable(20, 2, 20)
for rep in range(3):
    eng.sample_begin()
    eng.push_reads(0, words, lens)
    eng.sample_finalize(1)
    eng.sample_junctions(1)
    jsum = eng.download_junctions(cap=0)[0]
    eng.sample_breakends(1)
    bsum = eng.download_breakends(cap=0)[0]
print("share %g: %d records; junctions: %d anchored, %d reference-spanning" % (SHARE, jsum.records, jsum.anchored, jsum.ref_spanning))
print("breakends: %d with one anchor, %d reference-spanning, %d supporting, %d short, %d through, %d discordant, %d unplaced, %d events" %
      (bsum.one_anchor, bsum.ref_spanning, bsum.supporting, bsum.short_, bsum.through, bsum.discordant, bsum.unplaced, bsum.candidates))
eng.close()
ix.close()
