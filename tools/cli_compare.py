#!/usr/bin/env python3
"""Two `bronko` binaries on the same generated argument vectors: any difference in exit code, stdout or stderr is reported (the
`finished in` line left out).  tools/cli_compare.py OLD NEW [SEED [N_RANDOM]].  Needs no GPU: a vector ends in parse_args (exit 2), in
check_call_args (exit 1) or, the few that pass every check, at "no HIP device" once tests/golden/hpv.bkdb is loaded.

Per option: absent, a valid value, just below and just above each bound, a non-number, a missing value, `--opt=value` beside
`--opt value`; then random pairs and triples of these.  All but a few vectors end with --mst, whose "--mst needs --distances" is one
of the last rules: what comes before it has passed every check without an index being loaded.  Values stay within a long: beyond it
--min-base-qual, --primer-mismatches and --adapter-min-overlap are now refused by the parser (exit 2) like every other integer."""
import os, random, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "hpv.bkdb")
M8, R1 = (0, 8), (1, None)                         # 0..8 mismatches, at least 1 read
# option -> (the switches that let it pass its "needs" rule, lo, hi or None, a valid value); reals are floats
INTS = {"--min-base-qual": ([], 0, 93, 20), "--primer-mismatches": (["--primers", "P"], 0, 3, 2), "--adapter-min-overlap": (["--adapter", "truseq"], 3, 13, 6),
        "--consensus-min-depth": (["--consensus"], 1, None, 5), "--region-window": ([], 1, None, 500), "--region-min-depth": (["--region-window", "400"], 1, None, 5),
        "--indel-max-len": (["--indels"], 1, 32, 8), "--indel-max-mismatches": (["--indels"], *M8, 1), "--indel-min-reads": (["--indels"], *R1, 3),
        "--junction-min-len": (["--junctions"], 1, (1 << 27) - 1, 50), "--junction-max-mismatches": (["--junctions"], *M8, 1), "--junction-min-reads": (["--junctions"], *R1, 3),
        "--copyback-max-mismatches": (["--copybacks"], *M8, 1), "--copyback-min-reads": (["--copybacks"], *R1, 3), "--copyback-min-dist": (["--copybacks"], 0, 0xffffffff, 7),
        "--chimera-max-mismatches": (["--chimeras"], *M8, 1), "--chimera-min-reads": (["--chimeras"], *R1, 3),
        "--breakend-min-clip": (["--breakends"], 16, 65519, 30), "--breakend-max-mismatches": (["--breakends"], *M8, 1), "--breakend-min-reads": (["--breakends"], *R1, 3),
        "--duplication-min-len": (["--duplications"], 1, (1 << 27) - 1, 50), "--duplication-max-mismatches": (["--duplications"], *M8, 1),
        "--duplication-min-reads": (["--duplications"], *R1, 3),
        "--link-max-mismatches": (["--linkage"], *M8, 8), "--link-max-dist": (["--linkage"], 1, 65519, 300), "--link-min-reads": (["--linkage"], *R1, 3),
        "--codon-min-reads": (["--codons", "B"], *R1, 3), "--codon-max-mismatches": (["--codons", "B"], *M8, 8),
        "--hap-window": ([], 1, 65520, 300), "--hap-step": (["--hap-window", "200"], 1, None, 100), "--hap-min-reads": (["--haplotypes", "B"], *R1, 3),
        "--hap-max-mismatches": (["--hap-window", "200"], *M8, 8), "--read-pileup-end": (["--read-pileup"], 0, 255, 5),
        "--read-pileup-max-mismatches": (["--read-pileup"], *M8, 8), "--clusters": (["--consensus", "--distances"], 0, None, 4),
        "--kmer-size": ([], 15, 31, 21), "--threads": ([], 1, None, 2), "--min-kmers": ([], 0, None, 2), "--n-fixed": ([], 0, None, 1), "--n-per-strand": ([], 0, 20, 3),
        "--min-depth": ([], 0, None, 10), "--min-variant-depth": ([], 0, None, 2)}
REALS = {"--adapter-error-rate": (["--adapter", "nextera"], 0.0, 0.3, 0.2), "--consensus-min-freq": (["--consensus"], 0.0, 1.0, 0.7),
         "--indel-min-af": (["--indels"], 0.0, 1.0, 0.1), "--codon-min-freq": (["--codons", "B"], 0.0, 1.0, 0.1), "--hap-min-freq": (["--hap-window", "90"], 0.0, 1.0, 0.1),
         "--cluster-min-breadth": (["--consensus", "--distances", "--clusters", "3"], 0.0, 1.0, 0.5), "--mst-min-breadth": (["--consensus", "--distances", "--mst"], 0.0, 1.0, 0.5),
         "--min-af": ([], 0.0, 1.0, 0.02), "--balance-ratio": ([], 0.0, 1.0, 0.3), "--noise-multiplier": ([], 1.0, 2.0, 1.2), "--strand_odds": ([], 0.0, None, 4.0)}
SWITCHES = ["--consensus", "--indels", "--consensus-indels", "--junctions", "--copybacks", "--chimeras", "--breakends", "--duplications", "--linkage", "--read-pileup",
            "--distances", "--mst", "--pileup", "--alignment", "--keep-kmer-info", "--use-full-kmer", "--no-end-filter", "--no-strand-filter", "--no-strand-balance-filter",
            "--debug", "--verbose", "--bogus", "-x", "--help=1", "-V"]
TEXTS = ["--primers", "--regions", "--codons", "--haplotypes", "--adapter", "--db", "-g", "-1", "-2", "-o", "--output"]
SHORT = {"--kmer-size": "-k", "--threads": "-t"}


def fragments(files):
    fix = lambda toks: [files.get(t, t) for t in toks]
    out = [[]]
    for table, step in ((INTS, 1), (REALS, 0.01)):
        for opt, (needs, lo, hi, ok) in table.items():
            values = [ok, lo, lo - step, "x", "", "-0", "1e3", "0x10"] + ([hi, hi + step] if hi is not None else [1 << 40])
            for v in values:
                out += [fix(needs) + [opt, str(v)], fix(needs) + ["%s=%s" % (opt, v)], [opt, str(v)]]
            out += [fix(needs) + [opt], [opt]]                                   # a missing value where it comes last
            if opt in SHORT:
                out += [[SHORT[opt] + str(ok)], [SHORT[opt] + "=" + str(ok)], [SHORT[opt], str(lo - 1)], [SHORT[opt]]]
    out += [[s] for s in SWITCHES] + [[s + "=1"] for s in SWITCHES[:4]]
    for t in TEXTS:
        out += [[t], [t, ""], [t + "="], [t, files["B"]], [t + "=" + files["P"]], [t, "no_such_file.fa"], [t, files["B"], files["P"]]]
    return out


def main():
    old, new, seed, n_random = sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1, int(sys.argv[4]) if len(sys.argv) > 4 else 3000
    rng = random.Random(seed)
    tmp = tempfile.mkdtemp(prefix="cli_compare_")
    files = {"B": os.path.join(tmp, "r.bed"), "P": os.path.join(tmp, "p.fa"), "FQ": os.path.join(tmp, "x.fastq")}
    open(files["B"], "w").write("HPV16\t0\t300\tE6\t0\t+\n")
    open(files["P"], "w").write(">p1\nACGTACGTACGTACGTAC\n")
    open(files["FQ"], "w").write("@a\nACGT\n+\nIIII\n")
    frags = fragments(files)
    head = ["call", "-d", DB, "-r", files["FQ"], "-o", os.path.join(tmp, "o")]
    vectors = [head + f + ["--mst"] for f in frags] + [head + f for f in frags[::40]]            # (the few that may reach the index)
    vectors += [head + sum(rng.sample(frags, rng.choice((2, 3))), []) + ["--mst"] for _ in range(n_random)]
    vectors += [["build", "-g", "no_such.fa", "-o", os.path.join(tmp, "ix")] + f for f in frags[::7]] + [[], ["call"], ["build"], ["--version"], ["help"], ["nonsense"]]

    def run(binary, v):
        r = subprocess.run([binary] + v, capture_output=True, text=True)
        return r.returncode, r.stdout, "\n".join(l for l in r.stderr.split("\n") if "finished in" not in l)
    with ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        both = list(pool.map(lambda v: (run(old, v), run(new, v)), vectors))
    differ = [(v, a, b) for v, (a, b) in zip(vectors, both) if a != b]
    for v, a, b in differ[:20]:
        print("DIFFERENT:", " ".join(v), "\n  old:", a, "\n  new:", b)
    ends = {}
    for a, _ in both:
        ends[a[0]] = ends.get(a[0], 0) + 1
    print("%d vectors (seed %d), exit codes of the old binary %s, %d reached the index, %d differences" %
          (len(vectors), seed, sorted(ends.items()), sum("no HIP device" in a[1] + a[2] for a, _ in both), len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
