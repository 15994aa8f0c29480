"""The texts with which the host twins and writers of the six anchor passes (--indels, --junctions, --copybacks, --duplications,
--chimeras, --breakends) refuse what they are given, word for word through hostlib: a report path that cannot be created or written,
a row outside the genome file, a genome file the index does not have, a parameter out of range.  No GPU."""
import os
import random

import pytest

from bronko_amd import hostlib
from bronko_amd.hostlib import HostIndex

K = 21
LEN_A, LEN_B = 300, 240
CELLS = LEN_A + LEN_B


@pytest.fixture(scope="module")
def ix():
    rng = random.Random(20261020)
    seqs = [("etA first", "".join(rng.choice("ACGT") for _ in range(LEN_A))), ("etB", "".join(rng.choice("ACGT") for _ in range(LEN_B)))]
    ix = HostIndex.build_mem(K, [("twins", [(name, s.encode()) for name, s in seqs])])
    assert ix.total_cells == CELLS
    yield ix
    ix.close()


def _text(fn, *args):
    with pytest.raises(RuntimeError) as err:
        fn(*args)
    return str(err.value)


# (the writer of hostlib with what follows `rows`, the word of its two file messages, a row outside the genome file, a row inside it)
WRITERS = {
    "indels": (lambda p, ix, f, rows: hostlib.write_indels_vcf(p, ix, f, "reads.fq", rows), "indel vcf", (CELLS, 3, 1, 0, 0, 0), (100, 3, 1, 0, 0, 0)),
    "junctions": (hostlib.write_junctions_tsv, "junctions", (CELLS, 40, 1, 0, 0, 0), (100, 40, 1, 0, 0, 0)),
    "copybacks": (hostlib.write_copybacks_tsv, "copybacks", (100, CELLS, 0, 1, 0, 0, 0, 0), (100, 160, 0, 1, 0, 0, 0, 0)),
    "duplications": (hostlib.write_duplications_tsv, "duplications", (CELLS + 5, 3, 1, 0, 0, 0), (100, 40, 1, 0, 0, 0)),
    "chimeras": (hostlib.write_chimeras_tsv, "chimeras", (100, CELLS, 0, 1, 0, 0, 0, 0), (100, LEN_A + 10, 0, 1, 0, 0, 0, 0)),
    "breakends": (hostlib.write_breakends_tsv, "breakends", (CELLS, 0, 0, 1, 0, 1, 0, 0), (100, 0, 0, 1, 0, 1, 0, 0)),
}
WRITER_NAME = {"indels": "write_indels_vcf", "junctions": "write_junctions_tsv", "copybacks": "write_copybacks_tsv",
               "duplications": "write_duplications_tsv", "chimeras": "write_chimeras_tsv", "breakends": "write_breakends_tsv"}


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_writer_refusals(ix, tmp_path, name):
    write, word, outside, inside = WRITERS[name]
    good = str(tmp_path / ("x." + name))
    write(good, ix, 0, [inside])                                     # the row inside is one: the refusals below are not the path's
    assert len(open(good).read().splitlines()) >= 2
    missing = str(tmp_path / "no_such_directory" / ("x." + name))
    assert _text(write, missing, ix, 0, []) == "bronko host: Failed to create %s output file %s" % (word, missing)
    assert not os.path.exists(os.path.dirname(missing))
    assert _text(write, good, ix, 0, [outside]) == "bronko host: %s: an event outside the genome file's sequences" % WRITER_NAME[name]
    no_file = "write_indels_vcf: no such genome file" if name == "indels" else "no such genome file"
    assert _text(write, good, ix, 1, []) == "bronko host: " + no_file
    assert _text(write, good, ix, -1, []) == "bronko host: " + no_file
    if os.path.exists("/dev/full"):                                  # a file that opens and takes nothing
        assert _text(write, "/dev/full", ix, 0, []) == "bronko host: Failed to write %s file /dev/full" % word


def test_chimera_writer_wants_two_sequences(ix, tmp_path):
    path = str(tmp_path / "x.chimeras.tsv")
    for row in ((100, 160, 0, 1, 0, 0, 0, 0), (LEN_A + 5, LEN_A + 90, 3, 0, 1, 0, 0, 0)):
        assert _text(hostlib.write_chimeras_tsv, path, ix, 0, [row]) == \
            "bronko host: write_chimeras_tsv: an event that does not join two sequences of the genome file"
    for row in ((160, 100, 0, 1, 0, 0, 0, 0), (100, 100, 0, 1, 0, 0, 0, 0), (100, LEN_A + 10, 4, 1, 0, 0, 0, 0)):
        assert _text(hostlib.write_chimeras_tsv, path, ix, 0, [row]) == "bronko host: write_chimeras_tsv: an event outside the genome file's sequences"


def test_other_rows_outside(ix, tmp_path):
    """The range checks that the first row of each writer above does not reach."""
    path = str(tmp_path / "x.tsv")
    for write, who, rows in (
            (hostlib.write_junctions_tsv, "write_junctions_tsv", [(0, 40, 1, 0, 0, 0), (LEN_A, 40, 1, 0, 0, 0), (LEN_A - 20, 40, 1, 0, 0, 0)]),
            (hostlib.write_copybacks_tsv, "write_copybacks_tsv", [(160, 100, 0, 1, 0, 0, 0, 0), (100, 160, 2, 1, 0, 0, 0, 0), (100, LEN_A + 10, 0, 1, 0, 0, 0, 0)]),
            (hostlib.write_duplications_tsv, "write_duplications_tsv", [(100, 0, 1, 0, 0, 0), (LEN_A + 10, 40, 1, 0, 0, 0)]),
            (hostlib.write_breakends_tsv, "write_breakends_tsv", [(100, 0, 2, 1, 0, 1, 0, 0)]),
            (lambda p, i, f, r: hostlib.write_indels_vcf(p, i, f, "reads.fq", r), "write_indels_vcf", [(0, 3, 1, 0, 0, 0), (LEN_A, -2, 1, 0, 0, 5), (LEN_A - 2, 3, 1, 0, 0, 0)])):
        for row in rows:
            assert _text(write, path, ix, 0, [row]) == "bronko host: %s: an event outside the genome file's sequences" % who, (who, row)


def test_parameters_out_of_range(ix):
    reads = ["ACGT"]
    for fn, args, word in (
            (hostlib.indel_events, (0, 2), "indel_events: max_len must be 1..32"),
            (hostlib.indel_events, (33, 2), "indel_events: max_len must be 1..32"),
            (hostlib.indel_events, (32, 9), "indel_events: max_mismatches must be 0..8"),
            (hostlib.indel_events, (32, -1), "indel_events: max_mismatches must be 0..8"),
            (hostlib.junction_events, (0, 2), "junction_events: min_len must be 1..2^27 - 1"),
            (hostlib.junction_events, (1 << 27, 2), "junction_events: min_len must be 1..2^27 - 1"),
            (hostlib.junction_events, (33, 9), "junction_events: max_mismatches must be 0..8"),
            (hostlib.copyback_events, (9,), "copyback_events: max_mismatches must be 0..8"),
            (hostlib.copyback_events, (-1,), "copyback_events: max_mismatches must be 0..8"),
            (hostlib.duplication_events, (0, 2), "duplication_events: min_len must be 1..2^27 - 1"),
            (hostlib.duplication_events, (1 << 27, 2), "duplication_events: min_len must be 1..2^27 - 1"),
            (hostlib.duplication_events, (33, 9), "duplication_events: max_mismatches must be 0..8"),
            (hostlib.chimera_events, (9,), "chimera_events: max_mismatches must be 0..8"),
            (hostlib.chimera_events, (-1,), "chimera_events: max_mismatches must be 0..8"),
            (hostlib.breakend_events, (15, 2), "breakend_events: min_clip must be 16..65519"),
            (hostlib.breakend_events, (65520, 2), "breakend_events: min_clip must be 16..65519"),
            (hostlib.breakend_events, (20, 9), "breakend_events: max_mismatches must be 0..8"),
            (hostlib.breakend_events, (15, 9), "breakend_events: max_mismatches must be 0..8")):
        assert _text(fn, ix, 0, reads, *args) == "bronko host: " + word, (fn.__name__, args)
    for fn in (hostlib.indel_events, hostlib.junction_events, hostlib.copyback_events, hostlib.duplication_events, hostlib.chimera_events,
               hostlib.breakend_events):
        assert _text(fn, ix, 1, reads) == "bronko host: no such genome file", fn.__name__
        rows, span, counters = fn(ix, 0, reads)                       # ... and within range: one read shorter than k is no record
        assert rows == [] and len(span) == CELLS and not span.any() and not any(counters)
