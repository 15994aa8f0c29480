"""What bk_last_error says of the six event passes (indels, junctions, copy-backs, chimeras, breakends, duplications) in the states
that one shared implementation of their lifecycle (bk_riders.cpp) words from a per-pass description: every text here is written out
whole, as include/bronko_hip.h's callers have seen it since each pass was added -- the nouns and the entry points' names follow no
one pattern, so none is built from one.  The chimera tests' crafted genome (it holds the other passes' crafted sequences) at k = 21,
300 records of 64 bases; the full table alone needs more than 2^10 distinct events, a record each."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from bronko_amd import BronkoError, _ffi, pack_reads
from bronko_amd.hostlib import HostIndex
from tests import breakend_cases, breakends_ref, chimera_cases, chimeras_ref, copyback_cases, copybacks_ref, duplication_cases, indel_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 21
INVALID, STATE = -1, -5

# pass -> (enable's arguments in front of table_log2, the summary's type, the texts)
PASSES = {
    "indels": ((32, 2), _ffi.IndelSummary, {
        "report_before_enable": "bk_sample_indels: indels were not enabled for this sample (bk_indels_enable before bk_sample_begin)",
        "enable_in_sample": "bk_indels_enable comes between samples",
        "download_before_report": "bk_sample_download_indels comes after this sample's bk_sample_indels",
        "span_room": "bk_sample_download_indel_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_indels: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_indels_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_indels_enable: the index has 2 genome files; indels are called against an index of one genome file",
        "full_table": "bk_sample_download_indels: more than 2^10 distinct candidate events: enable indels with a larger table_log2"}),
    "junctions": ((33, 2), _ffi.JunctionSummary, {
        "report_before_enable": "bk_sample_junctions: junctions were not enabled for this sample (bk_junctions_enable before bk_sample_begin)",
        "enable_in_sample": "bk_junctions_enable comes between samples",
        "download_before_report": "bk_sample_download_junctions comes after this sample's bk_sample_junctions",
        "span_room": "bk_sample_download_junction_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_junctions: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_junctions_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_junctions_enable: the index has 2 genome files; junctions are counted against an index of one genome file",
        "full_table": "bk_sample_download_junctions: more than 2^10 distinct candidate junctions: enable junctions with a larger table_log2"}),
    "copybacks": ((2,), _ffi.CopybackSummary, {
        "report_before_enable": "bk_sample_copybacks: copy-backs were not enabled for this sample (bk_copybacks_enable before bk_sample_begin)",
        "enable_in_sample": "bk_copybacks_enable comes between samples",
        "download_before_report": "bk_sample_download_copybacks comes after this sample's bk_sample_copybacks",
        "span_room": "bk_sample_download_copyback_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_copybacks: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_copybacks_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_copybacks_enable: the index has 2 genome files; copy-backs are counted against an index of one genome file",
        "full_table": "bk_sample_download_copybacks: more than 2^10 distinct candidate copy-backs: enable copy-backs with a larger table_log2"}),
    "chimeras": ((2,), _ffi.ChimeraSummary, {
        "report_before_enable": "bk_sample_chimeras: chimeras were not enabled for this sample (bk_chimeras_enable before bk_sample_begin)",
        "enable_in_sample": "bk_chimeras_enable comes between samples",
        "download_before_report": "bk_sample_download_chimeras comes after this sample's bk_sample_chimeras",
        "span_room": "bk_sample_download_chimera_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_chimeras: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_chimeras_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_chimeras_enable: the index has 2 genome files; chimeras are counted between the sequences of an index of one genome file",
        "full_table": "bk_sample_download_chimeras: more than 2^10 distinct candidate chimeras: enable chimeras with a larger table_log2"}),
    "breakends": ((20, 2), _ffi.BreakendSummary, {
        "report_before_enable": "bk_sample_breakends: breakends were not enabled for this sample (bk_breakends_enable before bk_sample_begin)",
        "enable_in_sample": "bk_breakends_enable comes between samples",
        "download_before_report": "bk_sample_download_breakends comes after this sample's bk_sample_breakends",
        "span_room": "bk_sample_download_breakend_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_breakends: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_breakends_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_breakends_enable: the index has 2 genome files; breakends are counted against an index of one genome file",
        "full_table": "bk_sample_download_breakends: more than 2^10 distinct candidate breakends: enable breakends with a larger table_log2"}),
    "duplications": ((33, 2), _ffi.DuplicationSummary, {
        "report_before_enable": "bk_sample_duplications: duplications were not enabled for this sample (bk_duplications_enable before bk_sample_begin)",
        "enable_in_sample": "bk_duplications_enable comes between samples",
        "download_before_report": "bk_sample_download_duplications comes after this sample's bk_sample_duplications",
        "span_room": "bk_sample_download_duplication_span: room for 5 cells, the index has 6523",
        "min_reads_0": "bk_sample_duplications: min_reads must be at least 1, got 0",
        "table_log2_9": "bk_duplications_enable: table_log2 must be 10..24, got 9",
        "two_files": "bk_duplications_enable: the index has 2 genome files; duplications are counted against an index of one genome file",
        "full_table": "bk_sample_download_duplications: more than 2^10 distinct candidate duplications: enable duplications with a larger table_log2"}),
}
SPAN_DOWNLOAD = {"indels": "bk_sample_download_indel_span", "junctions": "bk_sample_download_junction_span",
                 "copybacks": "bk_sample_download_copyback_span", "chimeras": "bk_sample_download_chimera_span",
                 "breakends": "bk_sample_download_breakend_span", "duplications": "bk_sample_download_duplication_span"}


def event_reads(noun, text, first):
    """More than 2^10 records of 64 bases of the pass `noun`, each an event of its own (the restatements count 1,200 and more)."""
    rng = random.Random(7)
    if noun == "indels":                                  # distinct inserted sequences at one place
        pos, seqs = indel_cases._free_pos(text, 800, 1), set()
        while len(seqs) < 1200:
            s = indel_cases._rand(rng, 6)
            if s[-1] != text[pos - 1]:
                seqs.add(s)
        return [indel_cases.mut_read(text, pos - 29, 64, ins=(pos, s)) for s in sorted(seqs)]
    if noun == "junctions":
        return [indel_cases.mut_read(text, p - 32, 64, dele=(p, d)) for d in (40, 43, 47, 52) for p in range(100, 560)]
    if noun == "duplications":
        return [duplication_cases.dup_read(text, p, e, 32, 64) for e in (40, 43, 47, 52) for p in range(100, 560)]
    if noun == "copybacks":
        return [copyback_cases.turn_read(text, copybacks_ref.H if i % 2 else copybacks_ref.T, 100 + i % 450, 700 + (i * 7) % 500, 32, 32)
                for i in range(1400)]
    if noun == "chimeras":                                # out of craftE into craftF
        return [chimera_cases.chimera_read(text, first[4] + 100 + i % 700, chimeras_ref.L, first[5] + 100 + (i * 7) % 900, chimeras_ref.R, 32, 32)
                for i in range(1400)]
    cells = list(range(first[4] + 50, first[4] + 850)) + list(range(first[5] + 50, first[5] + 650))
    return [breakend_cases.clipped(text, rng, c, breakends_ref.L, 64, 30) for c in cells]


class World:
    def __init__(self):
        seqs = chimera_cases.crafted_genome(K)
        g = chimeras_ref.Genome([name.split()[0] for name, _ in seqs], [s for _, s in seqs], K)
        self.ix = HostIndex.build_mem(K, [("crafted", [(n, s.encode()) for n, s in seqs])])
        self.reads = {}
        for noun in PASSES:
            reads = event_reads(noun, g.text, g.first)
            assert len(reads) >= 1200 and {len(r) for r in reads} == {64}
            self.reads[noun] = pack_reads([r.encode() for r in reads], K), pack_reads([r.encode() for r in reads[:300]], K)
        self.ix2 = HostIndex.build(K, [os.path.join(GOLDEN, "4_sarscov2", n) for n in ("wuhan_ref.fasta", "OM223929.1.fasta")])


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ix.close()
    w.ix2.close()


def _error(eng, fn, *a):
    """(status, bk_last_error) of a call of the Python API that must fail"""
    with pytest.raises(BronkoError) as ei:
        fn(*a)
    return ei.value.status, eng._L.bk_last_error().decode()


@pytest.mark.parametrize("noun", list(PASSES))
def test_the_texts_of_the_call_order_and_the_parameters(world, noun):
    cfg, _, text = PASSES[noun]
    eng = world.ix.engine()
    enable, report, download = getattr(eng, noun + "_enable"), getattr(eng, "sample_" + noun), getattr(eng, "download_" + noun)
    try:
        assert eng.total_cells == 6523
        assert _error(eng, report, 1) == (STATE, text["report_before_enable"])
        assert _error(eng, enable, *cfg, 9) == (INVALID, text["table_log2_9"])
        enable(*cfg, 16)
        eng.sample_begin()
        assert _error(eng, enable, *cfg, 16) == (STATE, text["enable_in_sample"])
        eng.push_reads(0, *world.reads[noun][1])
        eng.sample_finalize(1)
        assert _error(eng, download) == (STATE, text["download_before_report"])
        assert _error(eng, report, 0) == (INVALID, text["min_reads_0"])
        report(1)
        room = np.zeros(8, np.uint32)
        assert getattr(eng._L, SPAN_DOWNLOAD[noun])(eng.h, room.ctypes.data_as(C.c_void_p), 5) == INVALID
        assert eng._L.bk_last_error().decode() == text["span_room"] and not room.any()
        summ, rows = download()                           # ... and none of them spoiled the sample
        assert summ.records == 300 and summ.overflow == 0 and summ.reported == len(rows) > 0
    finally:
        eng.close()


@pytest.mark.parametrize("noun", list(PASSES))
def test_the_text_of_an_index_of_two_genome_files(world, noun):
    cfg, _, text = PASSES[noun]
    eng = world.ix2.engine()
    try:
        assert _error(eng, getattr(eng, noun + "_enable"), *cfg, 16) == (INVALID, text["two_files"])
    finally:
        eng.close()


@pytest.mark.parametrize("noun", list(PASSES))
def test_the_text_of_a_full_table(world, noun):
    cfg, summary, text = PASSES[noun]
    eng = world.ix.engine()
    try:
        getattr(eng, noun + "_enable")(*cfg, 10)
        eng.sample_begin()
        eng.push_reads(0, *world.reads[noun][0])
        eng.sample_finalize(1)
        getattr(eng, "sample_" + noun)(1)
        summ = summary()
        assert getattr(eng._L, "bk_sample_download_" + noun)(eng.h, C.byref(summ), None, 0) == INVALID
        assert eng._L.bk_last_error().decode() == text["full_table"] and summ.overflow == 1
    finally:
        eng.close()
