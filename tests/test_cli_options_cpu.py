"""The surface of `bronko call`'s arguments, sentence by sentence: every "needs" rule, every range rule just outside each bound, the
parsing conventions, the order in which two violations are reported and the one-genome-file message of the ten reports that have it.
Every text is written out whole, as the binary has printed it since the option was added -- none is built from the option table or
the rule list (cli.cpp) that print them now.  Each run ends in parse_args (exit 2), in check_call_args (exit 1) or, for the last
test, as the index is opened: no run gets as far as a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_options")
    fq, bed = str(d / "x.fastq"), str(d / "r.bed")
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    open(bed, "w").write("NC_045512.2\t0\t300\torf\t0\t+\n")
    return {"fq": fq, "bed": bed, "out": str(d / "o"), "dir": d}


def call(files, *extra, db=None):
    return subprocess.run([BRONKO, "call", "-d", db or os.path.join(GOLDEN, "hpv.bkdb"), "-r", files["fq"], "-o", files["out"]] + list(extra),
                          capture_output=True, text=True)


def dies_with(r, message):
    """exit code 1, and the run's last line is the error, whole"""
    return r.returncode == 1 and r.stdout.split("\n")[-2:] == ["ERROR [bronko::call] " + message, ""] and "no HIP device" not in r.stdout


NEEDS = [  # the arguments (the option alone, with a valid value where it takes one) -> the sentence
    ("--primer-mismatches 1", "--primer-mismatches needs --primers"),
    ("--adapter-min-overlap 5", "--adapter-min-overlap needs --adapter"),
    ("--adapter-error-rate 0.1", "--adapter-error-rate needs --adapter"),
    ("--consensus-min-depth 5", "--consensus-min-depth needs --consensus"),
    ("--consensus-min-freq 0.5", "--consensus-min-freq needs --consensus"),
    ("--region-min-depth 5", "--region-min-depth needs --regions or --region-window"),
    ("--regions=", "--regions needs a BED file"),
    ("--indel-max-len 8", "--indel-max-len needs --indels"),
    ("--indel-max-mismatches 1", "--indel-max-mismatches needs --indels"),
    ("--indel-min-reads 3", "--indel-min-reads needs --indels"),
    ("--indel-min-af 0.1", "--indel-min-af needs --indels"),
    ("--consensus-indels", "--consensus-indels needs --consensus"),
    ("--consensus --consensus-indels", "--consensus-indels needs --indels"),
    ("--junction-min-len 50", "--junction-min-len needs --junctions"),
    ("--junction-max-mismatches 1", "--junction-max-mismatches needs --junctions"),
    ("--junction-min-reads 3", "--junction-min-reads needs --junctions"),
    ("--copyback-max-mismatches 1", "--copyback-max-mismatches needs --copybacks"),
    ("--copyback-min-reads 3", "--copyback-min-reads needs --copybacks"),
    ("--copyback-min-dist 7", "--copyback-min-dist needs --copybacks"),
    ("--chimera-max-mismatches 1", "--chimera-max-mismatches needs --chimeras"),
    ("--chimera-min-reads 3", "--chimera-min-reads needs --chimeras"),
    ("--breakend-min-clip 30", "--breakend-min-clip needs --breakends"),
    ("--breakend-max-mismatches 1", "--breakend-max-mismatches needs --breakends"),
    ("--breakend-min-reads 3", "--breakend-min-reads needs --breakends"),
    ("--duplication-min-len 50", "--duplication-min-len needs --duplications"),
    ("--duplication-max-mismatches 1", "--duplication-max-mismatches needs --duplications"),
    ("--duplication-min-reads 3", "--duplication-min-reads needs --duplications"),
    ("--link-max-mismatches 4", "--link-max-mismatches needs --linkage"),
    ("--link-max-dist 300", "--link-max-dist needs --linkage"),
    ("--link-min-reads 3", "--link-min-reads needs --linkage"),
    ("--codon-min-reads 3", "--codon-min-reads needs --codons"),
    ("--codon-min-freq 0.1", "--codon-min-freq needs --codons"),
    ("--codon-max-mismatches 4", "--codon-max-mismatches needs --codons"),
    ("--codons=", "--codons needs a BED file"),
    ("--hap-step 50", "--hap-step needs --hap-window"),
    ("--hap-min-reads 3", "--hap-min-reads needs --haplotypes or --hap-window"),
    ("--hap-min-freq 0.1", "--hap-min-freq needs --haplotypes or --hap-window"),
    ("--hap-max-mismatches 4", "--hap-max-mismatches needs --haplotypes or --hap-window"),
    ("--haplotypes=", "--haplotypes needs a BED file"),
    ("--read-pileup-end 5", "--read-pileup-end needs --read-pileup"),
    ("--read-pileup-max-mismatches 4", "--read-pileup-max-mismatches needs --read-pileup"),
    ("--distances", "--distances needs --consensus"),
    ("--clusters 3", "--clusters needs --distances"),
    ("--cluster-min-breadth 0.5", "--cluster-min-breadth needs --clusters"),
    ("--mst", "--mst needs --distances"),
    ("--mst-min-breadth 0.5", "--mst-min-breadth needs --mst"),
]

RANGES = [  # the arguments: what lets the option pass its "needs" rule, then the option just outside a bound -> the sentence
    ("--min-base-qual -1", "Minimum base quality must be between 0 and 93 (Phred+33), got -1"),
    ("--min-base-qual 94", "Minimum base quality must be between 0 and 93 (Phred+33), got 94"),
    ("--primers P --primer-mismatches -1", "Primer mismatches must be between 0 and 3, got -1"),
    ("--primers P --primer-mismatches 4", "Primer mismatches must be between 0 and 3, got 4"),
    ("--consensus --consensus-min-depth 0", "Consensus minimum depth must be at least 1, got 0"),
    ("--consensus --consensus-min-freq -0.1", "Consensus minimum frequency must be between 0 and 1, got -0.1"),
    ("--consensus --consensus-min-freq 1.5", "Consensus minimum frequency must be between 0 and 1, got 1.5"),
    ("--region-window 0", "Region window must be at least 1, got 0"),
    ("--region-window 100 --region-min-depth 0", "Region minimum depth must be at least 1, got 0"),
    ("--indels --indel-max-len 0", "--indel-max-len must be between 1 and 32, got 0"),
    ("--indels --indel-max-len 33", "--indel-max-len must be between 1 and 32, got 33"),
    ("--indels --indel-max-mismatches -1", "--indel-max-mismatches must be between 0 and 8, got -1"),
    ("--indels --indel-max-mismatches 9", "--indel-max-mismatches must be between 0 and 8, got 9"),
    ("--indels --indel-min-reads 0", "--indel-min-reads must be at least 1, got 0"),
    ("--indels --indel-min-af -0.5", "--indel-min-af must be between 0 and 1, got -0.5"),
    ("--indels --indel-min-af 1.25", "--indel-min-af must be between 0 and 1, got 1.25"),
    ("--junctions --junction-min-len 0", "--junction-min-len must be between 1 and 134217727, got 0"),
    ("--junctions --junction-min-len 134217728", "--junction-min-len must be between 1 and 134217727, got 134217728"),
    ("--junctions --junction-max-mismatches -1", "--junction-max-mismatches must be between 0 and 8, got -1"),
    ("--junctions --junction-max-mismatches 9", "--junction-max-mismatches must be between 0 and 8, got 9"),
    ("--junctions --junction-min-reads 0", "--junction-min-reads must be at least 1, got 0"),
    ("--copybacks --copyback-max-mismatches -1", "--copyback-max-mismatches must be between 0 and 8, got -1"),
    ("--copybacks --copyback-max-mismatches 9", "--copyback-max-mismatches must be between 0 and 8, got 9"),
    ("--copybacks --copyback-min-reads 0", "--copyback-min-reads must be at least 1, got 0"),
    ("--copybacks --copyback-min-dist -1", "--copyback-min-dist must be between 0 and 4294967295, got -1"),
    ("--copybacks --copyback-min-dist 4294967296", "--copyback-min-dist must be between 0 and 4294967295, got 4294967296"),
    ("--chimeras --chimera-max-mismatches -1", "--chimera-max-mismatches must be between 0 and 8, got -1"),
    ("--chimeras --chimera-max-mismatches 9", "--chimera-max-mismatches must be between 0 and 8, got 9"),
    ("--chimeras --chimera-min-reads 0", "--chimera-min-reads must be at least 1, got 0"),
    ("--breakends --breakend-min-clip 15", "--breakend-min-clip must be between 16 and 65519, got 15"),
    ("--breakends --breakend-min-clip 65520", "--breakend-min-clip must be between 16 and 65519, got 65520"),
    ("--breakends --breakend-max-mismatches -1", "--breakend-max-mismatches must be between 0 and 8, got -1"),
    ("--breakends --breakend-max-mismatches 9", "--breakend-max-mismatches must be between 0 and 8, got 9"),
    ("--breakends --breakend-min-reads 0", "--breakend-min-reads must be at least 1, got 0"),
    ("--duplications --duplication-min-len 0", "--duplication-min-len must be between 1 and 134217727, got 0"),
    ("--duplications --duplication-min-len 134217728", "--duplication-min-len must be between 1 and 134217727, got 134217728"),
    ("--duplications --duplication-max-mismatches -1", "--duplication-max-mismatches must be between 0 and 8, got -1"),
    ("--duplications --duplication-max-mismatches 9", "--duplication-max-mismatches must be between 0 and 8, got 9"),
    ("--duplications --duplication-min-reads 0", "--duplication-min-reads must be at least 1, got 0"),
    ("--linkage --link-max-mismatches -1", "--link-max-mismatches must be between 0 and 8, got -1"),
    ("--linkage --link-max-mismatches 9", "--link-max-mismatches must be between 0 and 8, got 9"),
    ("--linkage --link-max-dist 0", "--link-max-dist must be between 1 and 65519, got 0"),
    ("--linkage --link-max-dist 65520", "--link-max-dist must be between 1 and 65519, got 65520"),
    ("--linkage --link-min-reads 0", "--link-min-reads must be at least 1, got 0"),
    ("--codons B --codon-min-reads 0", "--codon-min-reads must be at least 1, got 0"),
    ("--codons B --codon-max-mismatches -1", "--codon-max-mismatches must be between 0 and 8, got -1"),
    ("--codons B --codon-max-mismatches 9", "--codon-max-mismatches must be between 0 and 8, got 9"),
    ("--codons B --codon-min-freq -0.1", "--codon-min-freq must be between 0 and 1, got -0.1"),
    ("--codons B --codon-min-freq 1.1", "--codon-min-freq must be between 0 and 1, got 1.1"),
    ("--hap-window 0", "--hap-window must be between 1 and 65520, got 0"),
    ("--hap-window 65521", "--hap-window must be between 1 and 65520, got 65521"),
    ("--hap-window 100 --hap-step 0", "--hap-step must be at least 1, got 0"),
    ("--haplotypes B --hap-min-reads 0", "--hap-min-reads must be at least 1, got 0"),
    ("--haplotypes B --hap-max-mismatches -1", "--hap-max-mismatches must be between 0 and 8, got -1"),
    ("--hap-window 100 --hap-max-mismatches 9", "--hap-max-mismatches must be between 0 and 8, got 9"),
    ("--hap-window 100 --hap-min-freq -0.1", "--hap-min-freq must be between 0 and 1, got -0.1"),
    ("--haplotypes B --hap-min-freq 1.1", "--hap-min-freq must be between 0 and 1, got 1.1"),
    ("--read-pileup --read-pileup-end -1", "--read-pileup-end must be between 0 and 255, got -1"),
    ("--read-pileup --read-pileup-end 256", "--read-pileup-end must be between 0 and 255, got 256"),
    ("--read-pileup --read-pileup-max-mismatches -1", "--read-pileup-max-mismatches must be between 0 and 8, got -1"),
    ("--read-pileup --read-pileup-max-mismatches 9", "--read-pileup-max-mismatches must be between 0 and 8, got 9"),
    ("--consensus --distances --clusters -1", "--clusters must be at least 0, got -1"),
    ("--consensus --distances --clusters 3 --cluster-min-breadth -0.1", "--cluster-min-breadth must be between 0 and 1, got -0.1"),
    ("--consensus --distances --clusters 3 --cluster-min-breadth 1.1", "--cluster-min-breadth must be between 0 and 1, got 1.1"),
    ("--consensus --distances --mst --mst-min-breadth -0.1", "--mst-min-breadth must be between 0 and 1, got -0.1"),
    ("--consensus --distances --mst --mst-min-breadth 1.1", "--mst-min-breadth must be between 0 and 1, got 1.1"),
]

ORDER = [  # two violations: the first in the order of the checks is the one reported
    ("--indels --indel-min-af 2 --link-max-dist 0", "--link-max-dist needs --linkage"),
    ("--junction-min-len 0 --copyback-min-reads 0", "--junction-min-len needs --junctions"),
    ("--indels --linkage --indel-min-af 2 --link-max-dist 0", "--link-max-dist must be between 1 and 65519, got 0"),
    ("--indels --indel-min-af 2 --codon-min-reads 3", "--indel-min-af must be between 0 and 1, got 2"),
    ("--regions B --region-window 5 --region-min-depth 0", "--regions and --region-window cannot be given together"),
    ("--primer-mismatches 1 --min-base-qual 94", "Minimum base quality must be between 0 and 93 (Phred+33), got 94"),
    ("--consensus-indels --indels --indel-max-len 0", "--indel-max-len must be between 1 and 32, got 0"),
    ("--mst-min-breadth 2 --mst", "--mst needs --distances"),
    ("--linkage --link-max-mismatches 3 --codons B --codon-min-freq 2", "--codon-min-freq must be between 0 and 1, got 2"),
    ("--linkage --link-max-mismatches 3 --codons B --hap-step 4",
     "--linkage and --codons count the same placed reads: --link-max-mismatches (3) and --codon-max-mismatches (8) must be equal"),
    ("--haplotypes B --hap-window 0", "--haplotypes and --hap-window cannot be given together"),
    ("--read-pileup --read-pileup-max-mismatches 5 --hap-window 100 --distances",
     "--haplotypes and --read-pileup count the same placed reads: --hap-max-mismatches (8) and --read-pileup-max-mismatches (5) must be equal"),
]


def _args(files, text):
    return [files["bed"] if t == "B" else str(files["dir"] / "primers.fa") if t == "P" else t for t in text.split(" ")]


@pytest.mark.parametrize("args,sentence", NEEDS, ids=[a for a, _ in NEEDS])
def test_every_needs_sentence(files, args, sentence):
    r = call(files, *_args(files, args))
    assert dies_with(r, sentence), r.stdout


@pytest.mark.parametrize("args,sentence", RANGES, ids=[a for a, _ in RANGES])
def test_every_range_sentence_just_outside_its_bound(files, args, sentence):
    r = call(files, *_args(files, args))
    assert dies_with(r, sentence), r.stdout


@pytest.mark.parametrize("args,sentence", ORDER, ids=[a for a, _ in ORDER])
def test_of_two_violations_the_first_in_the_order_of_the_checks_is_reported(files, args, sentence):
    r = call(files, *_args(files, args))
    assert dies_with(r, sentence), r.stdout


def test_the_parsing_conventions(files):
    odd = "Invalid kmer size, must be odd and between [15-31]"
    for form in (["-k22"], ["-k=22"], ["-k", "22"], ["--kmer-size=22"], ["--kmer-size", "22"]):          # the value arrives in every form
        assert dies_with(call(files, *form), odd), form
    for form in (["-k21"], ["-k=21"], ["--kmer-size=21"], ["--indels", "--indel-max-len=8"], ["--adapter=truseq", "--adapter-min-overlap=6"]):
        assert dies_with(call(files, *form, "--mst"), "--mst needs --distances"), form
    assert dies_with(call(files, "--indels", "--indel-max-len=33"), "--indel-max-len must be between 1 and 32, got 33")

    def refused(r, text):     # the parser's own errors: exit 2, one line on stderr, nothing of the run on stdout but the banner
        return r.returncode == 2 and r.stderr == text + "\n" and "ERROR" not in r.stdout
    assert refused(call(files, "--indels", "--indel-max-len"), "error: a value is required for '--indel-max-len'")
    assert refused(call(files, "--min-af"), "error: a value is required for '--min-af'")
    assert refused(call(files, "--adapter"), "error: a value is required for '--adapter'")
    assert refused(call(files, "--adapter", "--consensus"), "error: a value is required for '--adapter'")
    assert refused(call(files, "-t"), "error: a value is required for '-t'")
    assert refused(call(files, "--indels", "--indel-max-len", "x"), "error: invalid value 'x' for '--indel-max-len'")
    assert refused(call(files, "--min-base-qual", "3q"), "error: invalid value '3q' for '--min-base-qual'")
    assert refused(call(files, "--primer-mismatches="), "error: invalid value '' for '--primer-mismatches'")
    assert refused(call(files, "--min-af", "half"), "error: invalid value 'half' for '--min-af'")
    assert refused(call(files, "-kx"), "error: invalid value 'x' for '-k'")
    assert refused(call(files, "--min-depth", "-1"), "error: invalid value '-1' for '--min-depth'")      # no negative number where none was ever taken
    assert refused(call(files, "-t", "-2"), "error: invalid value '-2' for '-t'")
    assert refused(call(files, "--n-fixed=-1"), "error: invalid value '-1' for '--n-fixed'")
    assert dies_with(call(files, "--indels", "--indel-min-reads", "-1"), "--indel-min-reads must be at least 1, got -1")   # ... and a sentence where one was
    assert dies_with(call(files, "--adapter", "truseq", "--adapter-min-overlap", "-4"),
                     "Adapter minimum overlap must be between 3 and the shortest adapter's length (13), got -4")
    assert refused(call(files, "--bogus"), "error: unexpected argument '--bogus' found")
    assert refused(call(files, "--bogus=3"), "error: unexpected argument '--bogus' found")
    assert refused(call(files, "-x"), "error: unexpected argument '-x' found")
    for opt in ("--indels", "--db", "--min-af", "-r", "--mst-min-breadth"):                               # a `call` option given to `build`
        r = subprocess.run([BRONKO, "build", "-g", "x.fa", opt], capture_output=True, text=True)
        assert refused(r, "error: unexpected argument '%s' found" % opt), opt


ONE_FILE = [
    ("--indels", "--indels needs an index of one genome file, this one has 2"),
    ("--junctions", "--junctions needs an index of one genome file, this one has 2"),
    ("--copybacks", "--copybacks needs an index of one genome file, this one has 2"),
    ("--chimeras", "--chimeras needs an index of one genome file, this one has 2"),
    ("--breakends", "--breakends needs an index of one genome file, this one has 2"),
    ("--duplications", "--duplications needs an index of one genome file, this one has 2"),
    ("--linkage", "--linkage needs an index of one genome file, this one has 2"),
    ("--codons B", "--codons needs an index of one genome file, this one has 2"),
    ("--haplotypes B", "--haplotypes needs an index of one genome file, this one has 2"),
    ("--hap-window 100", "--haplotypes needs an index of one genome file, this one has 2"),       # (the tiling is the same report)
    ("--read-pileup", "--read-pileup needs an index of one genome file, this one has 2"),
    ("--read-pileup --chimeras --junctions", "--junctions needs an index of one genome file, this one has 2"),   # (of several the first in their order)
]


@pytest.fixture(scope="module")
def two_genomes(files, sars_paths):
    stem = str(files["dir"] / "two")
    r = subprocess.run([BRONKO, "build", "-g", sars_paths[0], sars_paths[1], "-t", "2", "-o", stem], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    return stem + ".bkdb"


@pytest.mark.parametrize("args,sentence", ONE_FILE, ids=[a for a, _ in ONE_FILE])
def test_the_one_genome_file_sentence(files, two_genomes, args, sentence):
    r = call(files, *_args(files, args), db=two_genomes)
    assert dies_with(r, sentence), r.stdout
