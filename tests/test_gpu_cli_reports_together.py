"""Every per-sample report of `bronko call` in one run against each of them in a run of its own: the call driver runs the reports from
one description each (call_run.cpp), and a report must neither see nor disturb the others.  One single-end sample against
tests/golden/hpv.bkdb -- the linkage tests' planted sample with some of the indel and the junction tests' reads, 3,600 in all --, once
with every report on, then once per report with that report alone (and --consensus, --indels where it needs them): every file the solo
run wrote is byte-identical to the combined run's file of that name, and its summary line stands verbatim in the combined run's log."""
import os
import subprocess

import pytest

from tests import indel_cases, indels_ref, junction_cases, linkage_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRONKO = os.path.join(ROOT, "bronko_amd", "bin", "bronko")
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEM = "together"

# report -> (its flags, the start of its summary line, the files it writes beside the VCF and the overview)
REPORTS = {
    "pileup": (["--pileup"], "Writing output to pileup", [".tsv"]),
    "consensus": (["--consensus"], "Consensus of ", [".consensus.fa"]),
    "indels": (["--indels"], "Indels: ", [".indels.vcf"]),
    "consensus_indels": (["--consensus", "--indels", "--consensus-indels"], "Consensus indels: ", [".consensus.fa", ".consensus_indels.tsv", ".indels.vcf"]),
    "junctions": (["--junctions"], "Junctions: ", [".junctions.tsv"]),
    "copybacks": (["--copybacks"], "Copy-backs: ", [".copybacks.tsv"]),
    "chimeras": (["--chimeras"], "Chimeras: ", [".chimeras.tsv"]),
    "breakends": (["--breakends"], "Breakends: ", [".breakends.tsv"]),
    "duplications": (["--duplications"], "Duplications: ", [".duplications.tsv"]),
    "linkage": (["--linkage"], "Linkage: ", [".linkage.tsv"]),
    "codons": (["--codons", "GENES"], "Codons: ", [".codons.tsv"]),
    "haplotypes": (["--haplotypes", "AMPLICONS"], "Haplotypes: ", [".haplotypes.tsv"]),
    "read_pileup": (["--read-pileup"], "Read pileup: ", [".read_pileup.tsv"]),
    "regions": (["--regions", "AMPLICONS"], "Depth of ", [".regions.tsv"]),
}
ALL = ["--pileup", "--consensus", "--indels", "--consensus-indels", "--junctions", "--copybacks", "--chimeras", "--breakends", "--duplications", "--linkage",
       "--codons", "GENES", "--haplotypes", "AMPLICONS", "--read-pileup", "--regions", "AMPLICONS"]


class Sample:
    def __init__(self, d):
        self.dir = d
        text = indels_ref.read_fasta(os.path.join(GOLDEN, "HPV16.fa"), 21).text
        reads = linkage_cases.sample_reads(text)[0] + indel_cases.sample_reads(text, n_reads=600)[0] + junction_cases.sample_reads(text, n_reads=1000)[0]
        assert len(reads) == 3600
        self.fastq = str(d / (STEM + ".fastq"))
        with open(self.fastq, "w") as f:
            for i, r in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
        self.beds = {"GENES": str(d / "genes.bed"), "AMPLICONS": str(d / "amplicons.bed")}
        with open(self.beds["GENES"], "w") as f:          # over the planted substitutions of the linkage sample, both strands
            f.write("HPV16REF\t1980\t2280\torfA\t0\t+\nHPV16REF\t1701\t2001\torfB\t0\t-\n")
        with open(self.beds["AMPLICONS"], "w") as f:
            f.write("HPV16REF\t1990\t2080\tampA\nHPV16REF\t2050\t2150\tampB\nHPV16REF\t2150\t2260\tampC\nHPV16REF\t600\t700\tampD\n")

    def run(self, name, flags):
        """(stdout, {file name: bytes}) of one run of the binary"""
        out = str(self.dir / name)
        res = subprocess.run([BRONKO, "call", "-d", os.path.join(GOLDEN, "hpv.bkdb"), "-r", self.fastq, "-o", out, "-t", "8"] + [self.beds.get(f, f) for f in flags],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout, {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


@pytest.fixture(scope="session")
def sample(tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("reports_together"))


@pytest.fixture(scope="session")
def together(sample):
    return sample.run("all", ALL)


def _data_lines(blob):
    return [l for l in blob.decode().split("\n") if l and not l.startswith("#")]


def test_the_combined_run_writes_every_file_and_they_hold_data(together):
    log, files = together
    want = {STEM + suffix for _, _, suffixes in REPORTS.values() for suffix in suffixes} | {STEM + ".vcf", "bronko_overview.tsv"}
    assert set(files) == want
    for report, (_, summary, _) in REPORTS.items():
        assert sum(l.startswith("INFO  [bronko::call] " + summary) for l in log.split("\n")) == 1, report
    # the comparison below is not one of headers: more lines than a column line (the VCF's begins '#')
    for suffix in (".indels.vcf", ".junctions.tsv", ".linkage.tsv", ".codons.tsv", ".haplotypes.tsv", ".read_pileup.tsv", ".regions.tsv"):
        assert len(_data_lines(files[STEM + suffix])) >= 2, (suffix, files[STEM + suffix][-300:])


@pytest.mark.parametrize("report", list(REPORTS))
def test_a_report_alone_writes_what_it_writes_among_all_the_others(sample, together, report):
    flags, summary, suffixes = REPORTS[report]
    log_all, files_all = together
    log, files = sample.run(report, flags)
    assert set(files) == {STEM + s for s in suffixes} | {STEM + ".vcf", "bronko_overview.tsv"}
    for name, blob in files.items():
        if report == "consensus" and name == STEM + ".consensus.fa":
            continue     # (in the combined run that file is --consensus-indels': the sample's indels applied; the consensus_indels case compares it)
        assert blob == files_all[name], name
    lines = [l for l in log.split("\n") if l.startswith("INFO  [bronko::call] " + summary)]
    assert len(lines) == 1 and lines[0] in log_all.split("\n"), lines
    if report == "consensus":        # ... and without them the letters are the reference's length, none left out or put in
        plain = b"".join(files[STEM + ".consensus.fa"].split(b"\n")[1:])
        applied = b"".join(files_all[STEM + ".consensus.fa"].split(b"\n")[1:])
        assert len(plain) == 7906 and plain != applied
