#!/usr/bin/env python3
"""Randomised parity of the passes that ride on a sample's records (--indels, --linkage, --codons, --haplotypes, --read-pileup and their row store):
the cases of tests/rider_fuzz.py -- k from 11 to 31, genomes of one to three sequences with repeats, reverse-complement repeats and N
runs, reads of 20 to 600 bases with substitutions, indels of 1 to 33 bases, chimeras and foreign reads, every push path -- through
the engine, or with --cpu through the host twins, against the Python restatements.  One line per mismatch with the seed, the iteration
and the case's parameters; FUZZ_VERBOSE prints a line per iteration.  Exit status 1 on any mismatch.  With --trim every case also draws
adapters and primers, rewrites some of its reads to carry them and sets both on the engine (--adapter, --primers under every pass).
A mismatch line that says seed=S it=I trim=T is run again alone by `fuzz_riders.py [--trim] 1 S I` (--trim where T is 1).
Usage: fuzz_riders.py [--cpu] [--trim] [iterations [seed0 [first iteration]]]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rider_fuzz

args = [a for a in sys.argv[1:] if a not in ("--cpu", "--trim")]
cpu, trim = "--cpu" in sys.argv[1:], "--trim" in sys.argv[1:]
iters = int(args[0]) if len(args) > 0 else 100
seed0 = int(args[1]) if len(args) > 1 else 1
first = int(args[2]) if len(args) > 2 else 0

if not cpu:   # the ascii_device push views torch tensors: torch initialises its HIP context before the engine library does (tests/conftest.py)
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda:0")
t0 = time.time()
ran, bad = rider_fuzz.run(seed0, first, iters, rider_fuzz.check_host if cpu else rider_fuzz.check_engine, verbose=bool(os.environ.get("FUZZ_VERBOSE")),
                          out=lambda line: print(line, flush=True), trim=trim)
print("seed %d, %d iterations from %d (%s%s), %d mismatches, %.0f s" % (seed0, ran, first, "host twins" if cpu else "engine", ", trimmed" if trim else "", len(bad),
                                                                        time.time() - t0))
sys.exit(1 if bad else 0)
