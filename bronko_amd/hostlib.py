"""ctypes binding of the C++ host code (libbronko_host.so): index build and .bkdb codec (product code)."""
import ctypes as C
import os

import numpy as np

from .engine import BUCKET_INFO_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbronko_host.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("bronko_amd: %s is missing -- build it with `make -C bronko_amd/host`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.bh_last_error.restype = C.c_char_p
    L.bh_index_build.restype = vp
    L.bh_index_build.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int]
    L.bh_index_build_mem.restype = vp
    L.bh_index_build_mem.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                     C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int]
    L.bh_index_load.restype = vp
    L.bh_index_load.argtypes = [C.c_char_p]
    L.bh_index_save.restype = C.c_int
    L.bh_index_save.argtypes = [vp, C.c_char_p]
    L.bh_index_free.argtypes = [vp]
    for n, rt in (("bh_index_k", C.c_int), ("bh_index_meta_k", C.c_int), ("bh_index_n_buckets", C.c_uint64),
                  ("bh_index_n_entries", C.c_uint64), ("bh_index_bucket_ids", C.POINTER(C.c_uint64)),
                  ("bh_index_bucket_off", C.POINTER(C.c_uint64)), ("bh_index_entries", C.POINTER(C.c_uint8)),
                  ("bh_index_n_files", C.c_int), ("bh_index_total_cells", C.c_uint64)):
        getattr(L, n).restype = rt
        getattr(L, n).argtypes = [vp]
    L.bh_index_file_name.restype = C.c_char_p
    L.bh_index_file_name.argtypes = [vp, C.c_int]
    L.bh_index_n_seqs.restype = C.c_int
    L.bh_index_n_seqs.argtypes = [vp, C.c_int]
    L.bh_index_seq_name.restype = C.c_char_p
    L.bh_index_seq_name.argtypes = [vp, C.c_int, C.c_int]
    L.bh_index_seq_len.restype = C.c_uint64
    L.bh_index_seq_len.argtypes = [vp, C.c_int, C.c_int]
    L.bh_index_seq.restype = C.POINTER(C.c_uint8)
    L.bh_index_seq.argtypes = [vp, C.c_int, C.c_int]
    _lib = L
    return L


class HostIndex:
    """BronkoIndex (build.rs:23-28) held by the C++ host library."""

    def __init__(self, handle):
        L = load()
        if not handle:
            raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))
        self.h = C.c_void_p(handle)
        self.k = L.bh_index_k(self.h)
        self.meta_k = L.bh_index_meta_k(self.h)
        self.n_buckets = L.bh_index_n_buckets(self.h)
        self.n_entries = L.bh_index_n_entries(self.h)
        self.n_files = L.bh_index_n_files(self.h)
        self.total_cells = L.bh_index_total_cells(self.h)

    @classmethod
    def build(cls, k, fasta_paths, threads=4):
        arr = (C.c_char_p * len(fasta_paths))(*[p.encode() for p in fasta_paths])
        return cls(load().bh_index_build(k, arr, len(fasta_paths), threads))

    @classmethod
    def build_mem(cls, k, files, threads=4):
        """files: [(file_name, [(seq_name, seq_bytes), ...]), ...]"""
        fn = (C.c_char_p * len(files))(*[f[0].encode() for f in files])
        ns = (C.c_int * len(files))(*[len(f[1]) for f in files])
        flat = [s for f in files for s in f[1]]
        sn = (C.c_char_p * len(flat))(*[s[0].encode() for s in flat])
        sq = (C.c_char_p * len(flat))(*[bytes(s[1]) for s in flat])
        sl = (C.c_uint64 * len(flat))(*[len(s[1]) for s in flat])
        return cls(load().bh_index_build_mem(k, len(files), fn, ns, sn, sq, sl, threads))

    @classmethod
    def load(cls, path):
        return cls(load().bh_index_load(path.encode()))

    def save(self, path):
        L = load()
        if L.bh_index_save(self.h, path.encode()) != 0:
            raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))

    def close(self):
        if self.h:
            load().bh_index_free(self.h)
            self.h = None

    def bucket_ids(self):
        if not self.n_buckets:   # (an index of no k-mer at all: the empty vector's data() may be null)
            return np.zeros(0, np.uint64)
        return np.ctypeslib.as_array(load().bh_index_bucket_ids(self.h), shape=(self.n_buckets,)).copy()

    def bucket_off(self):
        return np.ctypeslib.as_array(load().bh_index_bucket_off(self.h), shape=(self.n_buckets + 1,)).copy()

    def entries(self):
        if not self.n_entries:
            return np.zeros(0, BUCKET_INFO_DTYPE)
        raw = np.ctypeslib.as_array(load().bh_index_entries(self.h), shape=(max(self.n_entries, 1) * 12,))
        return raw[: self.n_entries * 12].copy().view(BUCKET_INFO_DTYPE)

    def files(self):
        L = load()
        out = []
        for f in range(self.n_files):
            seqs = []
            for s in range(L.bh_index_n_seqs(self.h, f)):
                n = L.bh_index_seq_len(self.h, f, s)
                seq = bytes(np.ctypeslib.as_array(L.bh_index_seq(self.h, f, s), shape=(n,))) if n else b""
                seqs.append((L.bh_index_seq_name(self.h, f, s).decode(), seq))
            out.append((L.bh_index_file_name(self.h, f).decode(), seqs))
        return out

    def genome_len(self, f):
        L = load()
        return sum(L.bh_index_seq_len(self.h, f, s) for s in range(L.bh_index_n_seqs(self.h, f)))

    def engine(self, params=None):
        """bk_engine_create on this index."""
        from .engine import Engine
        return Engine(self.k, self.bucket_ids(), self.bucket_off(), self.entries(), self.files(), params)


class CallParams(C.Structure):  # bh_call_params == bronko::CallParams (cli.rs:92-135 defaults from consts.rs)
    _fields_ = [("k", C.c_int32), ("min_af", C.c_double), ("no_end_filter", C.c_int32), ("no_strand_filter", C.c_int32),
                ("no_strand_balance_filter", C.c_int32), ("strand_balance_ratio", C.c_double), ("n_per_strand", C.c_uint64),
                ("strand_odds_max", C.c_double), ("min_depth", C.c_uint64), ("min_variant_depth", C.c_uint64),
                ("variant_multiplier", C.c_double)]


def default_call_params(k=21):
    return CallParams(k, 0.03, 0, 0, 0, 0.1, 2, 6.0, 300, 3, 1.5)


def _caller_lib():
    L = load()
    if not hasattr(L, "_caller_ready"):
        vp = C.c_void_p
        L.bh_pick_best_genome.restype = C.c_int
        L.bh_pick_best_genome.argtypes = [vp, vp, vp]
        L.bh_baseline_noise_max.restype = None
        L.bh_baseline_noise_max.argtypes = [vp, vp, C.c_uint64, vp]
        L.bh_call_and_write.restype = C.c_int
        L.bh_call_and_write.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.POINTER(CallParams), C.c_char_p, C.c_char_p, C.c_char_p, vp, vp]
        L.bh_write_kmer_counts.restype = C.c_int
        L.bh_write_kmer_counts.argtypes = [C.c_char_p, C.c_int, vp, vp, C.c_uint64, C.c_int]
        L.bh_consensus.restype = C.c_int
        L.bh_consensus.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, C.c_double, vp, vp]
        L.bh_write_consensus_fasta.restype = C.c_int
        L.bh_write_consensus_fasta.argtypes = [vp, C.c_int, C.c_char_p, C.c_char_p, vp, C.c_uint64]
        u64 = C.c_uint64
        L.bh_bed_regions.restype = C.c_int
        L.bh_bed_regions.argtypes = [vp, C.c_char_p, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bh_window_regions.restype = C.c_int
        L.bh_window_regions.argtypes = [vp, u64, u64, vp, C.POINTER(u64)]
        L.bh_region_depths.restype = C.c_int
        L.bh_region_depths.argtypes = [vp, C.c_int, vp, vp, vp, u64, u64, vp, vp]
        L.bh_write_regions_tsv.restype = C.c_int
        L.bh_write_regions_tsv.argtypes = [vp, C.c_int, C.c_char_p, vp, C.c_char_p, u64, vp, u64, u64]
        L.bh_clean_sample_id.restype = None
        L.bh_clean_sample_id.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        L._caller_ready = True
    return L


def pick_best_genome(ix, stats, present):
    stats = np.ascontiguousarray(stats, np.uint64)
    present = np.ascontiguousarray(present, np.uint8)
    return _caller_lib().bh_pick_best_genome(ix.h, stats.ctypes.data, present.ctypes.data)


def baseline_noise_max(fwd4, rev4):
    fwd4 = np.ascontiguousarray(fwd4, np.uint64)
    rev4 = np.ascontiguousarray(rev4, np.uint64)
    out = np.zeros(len(fwd4) // 4)
    _caller_lib().bh_baseline_noise_max(fwd4.ctypes.data, rev4.ctypes.data, len(out), out.ctypes.data)
    return out


def call_and_write(ix, file_id, arrays, params, vcf_path=None, reads_path="", pileup_path=None):
    """call_variants + writers on four pileup arrays.  Returns (n_records, n_major, n_minor, breadth, depth)."""
    a = [np.ascontiguousarray(x, np.uint64) for x in arrays]
    summary = np.zeros(3, np.uint64)
    cov = np.zeros(2)
    L = _caller_lib()
    rc = L.bh_call_and_write(ix.h, file_id, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                             C.byref(params), vcf_path.encode() if vcf_path else None, reads_path.encode(),
                             pileup_path.encode() if pileup_path else None, summary.ctypes.data, cov.ctypes.data)
    if rc != 0:
        raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))
    return int(summary[0]), int(summary[1]), int(summary[2]), float(cov[0]), float(cov[1])


def clean_sample_id(path):
    buf = C.create_string_buffer(4096)
    _caller_lib().bh_clean_sample_id(path.encode(), buf, 4096)
    return buf.value.decode()


def write_kmer_counts(path, k, kmers, counts, threads=4):
    """The --keep-kmer-info writer (caller.cpp write_kmer_counts): "KMER\tCOUNT\n" per entry, in the order given."""
    km = np.ascontiguousarray(kmers, np.uint64)
    ct = np.ascontiguousarray(counts, np.uint64)
    assert len(km) == len(ct)
    L = _caller_lib()
    if L.bh_write_kmer_counts(path.encode(), k, km.ctypes.data, ct.ctypes.data, len(km), threads) != 0:
        raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))


def consensus(ix, file_id, fwd_depth, rev_depth, min_depth=10, min_freq=0.5):
    """The host twin of bk_sample_consensus (caller.cpp consensus) on the two depth arrays of all cells: (letters as bytes,
    (positions, called, ambiguous, masked, substitutions))."""
    fd = np.ascontiguousarray(fwd_depth, np.uint64)
    rd = np.ascontiguousarray(rev_depth, np.uint64)
    assert len(fd) == len(rd) == ix.total_cells * 4
    letters = np.zeros(max(1, ix.genome_len(file_id)), np.uint8)
    tallies = np.zeros(5, np.uint64)
    L = _caller_lib()
    if L.bh_consensus(ix.h, file_id, fd.ctypes.data, rd.ctypes.data, int(min_depth), float(min_freq), letters.ctypes.data, tallies.ctypes.data) != 0:
        raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))
    return letters[:int(tallies[0])].tobytes(), tuple(int(t) for t in tallies)


def write_consensus_fasta(path, stem, ix, file_id, letters):
    """The --consensus writer (caller.cpp write_consensus_fasta)."""
    buf = np.frombuffer(bytes(letters), np.uint8)
    L = _caller_lib()
    if L.bh_write_consensus_fasta(ix.h, file_id, path.encode(), stem.encode(), buf.ctypes.data if len(buf) else None, len(buf)) != 0:
        raise RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))


def _host_error(L):
    return RuntimeError("bronko host: " + L.bh_last_error().decode(errors="replace"))


def _region_array(regions):
    """[(file_id, seq, start, end, ...)] -> [n][4] u32 as the bh_* region functions take them"""
    return np.ascontiguousarray([tuple(r[:4]) for r in regions], np.uint32).reshape(len(regions), 4)


def bed_regions(ix, path):
    """A --regions BED file read and resolved against the index (caller.cpp read_bed, resolve_bed): [(file_id, seq, start, end, name)]
    in the file's order; RuntimeError with the file and the line named for what the file or the index refuses."""
    L = _caller_lib()
    n, nl = C.c_uint64(), C.c_uint64()
    if L.bh_bed_regions(ix.h, path.encode(), 0, None, None, 0, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    regs = np.zeros((max(1, n.value), 4), np.uint32)
    names = C.create_string_buffer(max(1, nl.value))
    if L.bh_bed_regions(ix.h, path.encode(), n.value, regs.ctypes.data, names, nl.value, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    nm = names.value.decode().split("\n") if n.value else []
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), nm[i]) for i, r in enumerate(regs[:n.value])]


def window_regions(ix, window):
    """--region-window W: [iW, min((i + 1)W, len)) over every sequence of every genome file (caller.cpp window_regions), named '.'."""
    L = _caller_lib()
    n = C.c_uint64()
    if L.bh_window_regions(ix.h, int(window), 0, None, C.byref(n)) != 0:
        raise _host_error(L)
    regs = np.zeros((max(1, n.value), 4), np.uint32)
    if L.bh_window_regions(ix.h, int(window), n.value, regs.ctypes.data, C.byref(n)) != 0:
        raise _host_error(L)
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), ".") for r in regs[:n.value]]


def region_depths(ix, file_id, fwd_depth, rev_depth, regions, min_depth=10):
    """The host twin of bk_sample_region_depths (caller.cpp region_depths) on the two depth arrays of all cells: (rows, (full,
    partial, empty)) with one (sum, min, max, median, covered) per region of `file_id` among `regions`, in order."""
    fd = np.ascontiguousarray(fwd_depth, np.uint64)
    rd = np.ascontiguousarray(rev_depth, np.uint64)
    assert len(fd) == len(rd) == ix.total_cells * 4
    regs = _region_array(regions)
    rows = np.zeros((max(1, len(regions)), 5), np.uint64)
    tallies = np.zeros(4, np.uint64)
    L = _caller_lib()
    if L.bh_region_depths(ix.h, file_id, fd.ctypes.data, rd.ctypes.data, regs.ctypes.data, len(regions), int(min_depth), rows.ctypes.data, tallies.ctypes.data) != 0:
        raise _host_error(L)
    return [tuple(int(v) for v in r) for r in rows[:int(tallies[0])]], tuple(int(t) for t in tallies[1:])


def write_regions_tsv(path, ix, file_id, regions, rows, min_depth):
    """The --regions writer (caller.cpp write_regions_tsv): regions as bed_regions gives them, rows of those of `file_id`."""
    regs = _region_array(regions)
    names = "\n".join(r[4] if len(r) > 4 else "." for r in regions).encode()
    rw = np.ascontiguousarray(rows, np.uint64).reshape(len(rows), 5)
    L = _caller_lib()
    if L.bh_write_regions_tsv(ix.h, file_id, path.encode(), regs.ctypes.data, names, len(regions), rw.ctypes.data, len(rows), int(min_depth)) != 0:
        raise _host_error(L)


# bk_indel_record (include/bronko_hip.h) == bronko::IndelEvent (indels.hpp)
INDEL_DTYPE = np.dtype([("cell", np.uint32), ("len", np.int32), ("fwd", np.uint32), ("rev", np.uint32), ("ref_span", np.uint32),
                        ("pad", np.uint32), ("seq", np.uint64)])


_VP, _U64, _U32 = C.c_void_p, C.c_uint64, C.c_uint32
_EVENTS_TAIL = [_U64, _VP, C.POINTER(_U64), _VP, _VP]      # what every bh_*_events ends with: cap, rows, n, span, counters


def _bound(ready, signatures):
    """The library with the argtypes of the bh_* functions of `signatures` ({name: argtypes}, each returning int) set, once."""
    L = _caller_lib()
    if not hasattr(L, ready):
        for name, argtypes in signatures.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, argtypes
        setattr(L, ready, True)
    return L


def _events(fn, ix, file_id, reads, params, shape, dtype, n_counters):
    """The two calls of a bh_*_events over ASCII reads, the first for the table's size: (its records as an array of `dtype` with
    `shape` per record, the prefix-summed span array of all cells, the counters)."""
    joined = "\n".join(reads).encode()
    n = C.c_uint64()
    span = np.zeros(max(1, ix.total_cells), np.uint32)
    counters = np.zeros(n_counters, np.uint64)
    if fn(ix.h, file_id, joined, *params, 0, None, C.byref(n), None, None) != 0:
        raise _host_error(load())
    rec = np.zeros((max(1, n.value),) + shape, dtype)
    if fn(ix.h, file_id, joined, *params, n.value, rec.ctypes.data, C.byref(n), span.ctypes.data, counters.ctypes.data) != 0:
        raise _host_error(load())
    return rec[:n.value], span[:ix.total_cells], tuple(int(c) for c in counters)


def _u32_rows(rec):
    """[n][width] u32 as sorted tuples of int"""
    return sorted(tuple(int(v) for v in r) for r in rec)


def _u32_records(rows, width):
    """rows of `width` numbers each as the [n][width] u32 that a bh_write_* takes (one zero record for none)"""
    rec = np.zeros((max(1, len(rows)), width), np.uint32)
    for i, r in enumerate(rows):
        rec[i] = r
    return rec


def _indel_lib():
    return _bound("_indels_ready", {"bh_indel_events": [_VP, C.c_int, C.c_char_p, C.c_int, C.c_int] + _EVENTS_TAIL,
                                    "bh_write_indels_vcf": [_VP, C.c_int, C.c_char_p, C.c_char_p, _VP, _U64, _U32, _U32, _U64, _U32]})


def indel_rows(rec):
    """A structured array of bk_indel_record as [(cell, len, fwd, rev, ref_span, seq)] sorted by (cell, kind, length, seq)."""
    rows = [(int(r["cell"]), int(r["len"]), int(r["fwd"]), int(r["rev"]), int(r["ref_span"]), int(r["seq"])) for r in rec]
    rows.sort(key=lambda r: (r[0], 1 if r[1] < 0 else 0, abs(r[1]), r[5]))
    return rows


def indel_events(ix, file_id, reads, max_len=32, max_mismatches=2):
    """The host twin of the engine's indel pass (indels.cpp indel_events) over ASCII reads: (rows of the whole table as indel_rows
    gives them, the prefix-summed span array of all cells, (records, anchored, ref_spanning, supporting, discordant))."""
    rec, span, counters = _events(_indel_lib().bh_indel_events, ix, file_id, reads, (int(max_len), int(max_mismatches)), (), INDEL_DTYPE, 5)
    return indel_rows(rec), span, counters


def write_indels_vcf(path, ix, file_id, reads_path, rows, max_len=32, max_mismatches=2, min_reads=5, min_af_ppm=30000):
    """The --indels writer (indels.cpp write_indels_vcf): rows as indel_rows gives them, already filtered."""
    rec = np.zeros(max(1, len(rows)), INDEL_DTYPE)
    for i, r in enumerate(rows):
        rec[i] = (r[0], r[1], r[2], r[3], r[4], 0, r[5])
    L = _indel_lib()
    if L.bh_write_indels_vcf(ix.h, file_id, path.encode(), reads_path.encode(), rec.ctypes.data, len(rows), int(max_len), int(max_mismatches), int(min_reads),
                             int(min_af_ppm)) != 0:
        raise _host_error(L)


# bk_consensus_indel_record (include/bronko_hip.h) == bronko::ConsensusIndel (consensus_indels.hpp)
CONSENSUS_INDEL_DTYPE = np.dtype([("cell", np.uint32), ("len", np.int32), ("support", np.uint32), ("ref_span", np.uint32), ("seq", np.uint64),
                                  ("applied", np.uint32), ("pad", np.uint32)])
CONSENSUS_INDEL_TALLIES = ("candidates", "accepted", "applied", "contested", "deletions", "insertions", "deleted_bases", "inserted_bases", "frameshifts")


def _consensus_indel_lib():
    return _bound("_consensus_indels_ready", {
        "bh_consensus_indels": [_VP, C.c_int, _VP, _U64, _VP, _U64, C.c_double, _VP, _U64, _U64, _VP, C.POINTER(_U64), _VP],
        "bh_write_consensus_indels_fasta": [_VP, C.c_int, C.c_char_p, C.c_char_p, _VP, _U64, _VP, _U64],
        "bh_write_consensus_indels_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U64, C.c_double]})


def _consensus_indel_records(rows):
    """[(cell, len, support, ref_span, seq, applied)] as the array of bk_consensus_indel_record a bh_* takes (one zero record for none)"""
    rec = np.zeros(max(1, len(rows)), CONSENSUS_INDEL_DTYPE)
    for i, r in enumerate(rows):
        rec[i] = (r[0], r[1], r[2], r[3], r[4], r[5], 0)
    return rec


def consensus_indels(ix, file_id, events, span, letters, min_depth=10, min_freq=0.5):
    """The host twin of bk_sample_consensus_indels (consensus_indels.cpp): `events` as indel_rows gives the whole table, `span` the
    prefix-summed span array of all cells, `letters` the genome file's consensus letters.  Returns (the accepted events as
    [(cell, len, support, ref_span, seq, applied)] sorted by (cell, kind, length, seq), the tallies by name, the letters with '-' at
    the applied deletions)."""
    ev = np.zeros(max(1, len(events)), INDEL_DTYPE)
    for i, r in enumerate(events):
        ev[i] = (r[0], r[1], r[2], r[3], r[4], 0, r[5])
    sp = np.ascontiguousarray(span, np.uint32)
    assert len(sp) >= ix.total_cells
    out = np.frombuffer(bytes(letters), np.uint8).copy()
    rec = np.zeros(max(1, len(events)), CONSENSUS_INDEL_DTYPE)
    n, tallies = C.c_uint64(), np.zeros(len(CONSENSUS_INDEL_TALLIES), np.uint64)
    L = _consensus_indel_lib()
    if L.bh_consensus_indels(ix.h, file_id, ev.ctypes.data, len(events), sp.ctypes.data, int(min_depth), float(min_freq), out.ctypes.data if len(out) else None,
                             len(out), len(rec), rec.ctypes.data, C.byref(n), tallies.ctypes.data) != 0:
        raise _host_error(L)
    rows = [(int(r["cell"]), int(r["len"]), int(r["support"]), int(r["ref_span"]), int(r["seq"]), int(r["applied"])) for r in rec[:n.value]]
    return rows, dict(zip(CONSENSUS_INDEL_TALLIES, (int(t) for t in tallies))), out.tobytes()


def write_consensus_indels_fasta(path, stem, ix, file_id, letters, rows):
    """The --consensus-indels FASTA writer (consensus_indels.cpp write_consensus_indels_fasta): the letters with '-' at the applied
    deletions, rows as consensus_indels gives them."""
    buf = np.frombuffer(bytes(letters), np.uint8)
    rec = _consensus_indel_records(rows)
    L = _consensus_indel_lib()
    if L.bh_write_consensus_indels_fasta(ix.h, file_id, path.encode(), stem.encode(), buf.ctypes.data if len(buf) else None, len(buf), rec.ctypes.data, len(rows)) != 0:
        raise _host_error(L)


def write_consensus_indels_tsv(path, ix, file_id, rows, min_depth=10, min_freq=0.5):
    """The --consensus-indels table writer (consensus_indels.cpp write_consensus_indels_tsv)."""
    rec = _consensus_indel_records(rows)
    L = _consensus_indel_lib()
    if L.bh_write_consensus_indels_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(min_depth), float(min_freq)) != 0:
        raise _host_error(L)


def _junction_lib():
    return _bound("_junctions_ready", {"bh_junction_events": [_VP, C.c_int, C.c_char_p, _U32, C.c_int] + _EVENTS_TAIL,
                                       "bh_write_junctions_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U32, _U32, _U64]})


def junction_events(ix, file_id, reads, min_len=33, max_mismatches=2):
    """The host twin of the engine's junction pass (junctions.cpp junction_events) over ASCII reads: (rows of the whole table as
    bk_junction_record (cell, len, fwd, rev, span_donor, span_acceptor) sorted by (cell, len), the prefix-summed span array of all
    cells, (records, anchored, ref_spanning, supporting, short, backward, discordant))."""
    rec, span, counters = _events(_junction_lib().bh_junction_events, ix, file_id, reads, (int(min_len), int(max_mismatches)), (6,), np.uint32, 7)
    return _u32_rows(rec), span, counters


def write_junctions_tsv(path, ix, file_id, rows, min_len=33, max_mismatches=2, min_reads=5):
    """The --junctions writer (junctions.cpp write_junctions_tsv): rows as junction_events gives them, already filtered."""
    rec = _u32_records(rows, 6)
    L = _junction_lib()
    if L.bh_write_junctions_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(min_len), int(max_mismatches), int(min_reads)) != 0:
        raise _host_error(L)


def _copyback_lib():
    return _bound("_copybacks_ready", {"bh_copyback_events": [_VP, C.c_int, C.c_char_p, C.c_int] + _EVENTS_TAIL,
                                       "bh_write_copybacks_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U32, _U64, _U32]})


def copyback_events(ix, file_id, reads, max_mismatches=2):
    """The host twin of the engine's copy-back pass (copybacks.cpp copyback_events) over ASCII reads: (rows of the whole table as
    bk_copyback_record (lo, hi, kind, lo_first, hi_first, span_lo, span_hi, 0) sorted, the prefix-summed span array of all cells,
    (records, same_strand, ref_spanning, switched, supporting, discordant))."""
    rec, span, counters = _events(_copyback_lib().bh_copyback_events, ix, file_id, reads, (int(max_mismatches),), (8,), np.uint32, 6)
    return _u32_rows(rec), span, counters


def write_copybacks_tsv(path, ix, file_id, rows, max_mismatches=2, min_reads=5, min_dist=0):
    """The --copybacks writer (copybacks.cpp write_copybacks_tsv): rows as copyback_events gives them, already filtered."""
    rec = _u32_records(rows, 8)
    L = _copyback_lib()
    if L.bh_write_copybacks_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(max_mismatches), int(min_reads), int(min_dist)) != 0:
        raise _host_error(L)


def _chimera_lib():
    return _bound("_chimeras_ready", {"bh_chimera_events": [_VP, C.c_int, C.c_char_p, C.c_int] + _EVENTS_TAIL,
                                      "bh_write_chimeras_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U32, _U64, _U64, _U64]})


def chimera_events(ix, file_id, reads, max_mismatches=2):
    """The host twin of the engine's chimera pass (chimeras.cpp chimera_events) over ASCII reads: (rows of the whole table as
    bk_chimera_record (lo, hi, sides, lo_first, hi_first, span_lo, span_hi, 0) sorted, the prefix-summed span array of all cells,
    (records, same_strand, ref_spanning, crossed, supporting, discordant))."""
    rec, span, counters = _events(_chimera_lib().bh_chimera_events, ix, file_id, reads, (int(max_mismatches),), (8,), np.uint32, 6)
    return _u32_rows(rec), span, counters


def write_chimeras_tsv(path, ix, file_id, rows, max_mismatches=2, min_reads=5, supporting=0, ref_spanning=0):
    """The --chimeras writer (chimeras.cpp write_chimeras_tsv): rows as chimera_events gives them, already filtered, and the sample's
    two tallies that the header prints."""
    rec = _u32_records(rows, 8)
    L = _chimera_lib()
    if L.bh_write_chimeras_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(max_mismatches), int(min_reads), int(supporting), int(ref_spanning)) != 0:
        raise _host_error(L)


def _breakend_lib():
    return _bound("_breakends_ready", {"bh_breakend_events": [_VP, C.c_int, C.c_char_p, C.c_int, C.c_int] + _EVENTS_TAIL,
                                       "bh_write_breakends_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U32, _U32, _U64, _VP]})


def breakend_events(ix, file_id, reads, min_clip=20, max_mismatches=2):
    """The host twin of the engine's breakend pass (breakends.cpp breakend_events) over ASCII reads: (rows of the whole table as
    bk_breakend_record (cell, tag, side, fwd, rev, site_reads, span, 0) sorted, the prefix-summed span array of all cells,
    (records, one_anchor, ref_spanning, supporting, short, through, discordant, unplaced))."""
    rec, span, counters = _events(_breakend_lib().bh_breakend_events, ix, file_id, reads, (int(min_clip), int(max_mismatches)), (8,), np.uint32, 8)
    return _u32_rows(rec), span, counters


def write_breakends_tsv(path, ix, file_id, rows, min_clip=20, max_mismatches=2, min_reads=5, tallies=(0,) * 10):
    """The --breakends writer (breakends.cpp write_breakends_tsv): rows as breakend_events gives them, already filtered, and the
    sample's ten tallies (bk_breakend_summary's, without overflow) that the header prints."""
    rec = _u32_records(rows, 8)
    t = np.array([int(v) for v in tallies], np.uint64)
    assert t.shape == (10,)
    L = _breakend_lib()
    if L.bh_write_breakends_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(min_clip), int(max_mismatches), int(min_reads), t.ctypes.data) != 0:
        raise _host_error(L)


def _duplication_lib():
    return _bound("_duplications_ready", {"bh_duplication_events": [_VP, C.c_int, C.c_char_p, _U32, C.c_int] + _EVENTS_TAIL,
                                          "bh_write_duplications_tsv": [_VP, C.c_int, C.c_char_p, _VP, _U64, _U32, _U32, _U64]})


def duplication_events(ix, file_id, reads, min_len=33, max_mismatches=2):
    """The host twin of the engine's duplication pass (duplications.cpp duplication_events) over ASCII reads: (rows of the whole table as
    bk_duplication_record (cell, len, fwd, rev, span_start, span_end) sorted by (cell, len), the prefix-summed span array of all
    cells, (records, anchored, ref_spanning, supporting, short, forward, discordant))."""
    rec, span, counters = _events(_duplication_lib().bh_duplication_events, ix, file_id, reads, (int(min_len), int(max_mismatches)), (6,), np.uint32, 7)
    return _u32_rows(rec), span, counters


def write_duplications_tsv(path, ix, file_id, rows, min_len=33, max_mismatches=2, min_reads=5):
    """The --duplications writer (duplications.cpp write_duplications_tsv): rows as duplication_events gives them, already filtered."""
    rec = _u32_records(rows, 6)
    L = _duplication_lib()
    if L.bh_write_duplications_tsv(ix.h, file_id, path.encode(), rec.ctypes.data, len(rows), int(min_len), int(max_mismatches), int(min_reads)) != 0:
        raise _host_error(L)


def _link_lib():
    L = _caller_lib()
    if not hasattr(L, "_linkage_ready"):
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.bh_link_rows.restype = C.c_int
        L.bh_link_rows.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, u64, vp, C.POINTER(u64), vp]
        L.bh_link_count.restype = C.c_int
        L.bh_link_count.argtypes = [vp, C.c_int, vp, u64, vp, u64, u32, u64, vp, C.POINTER(u64)]
        L.bh_write_linkage_tsv.restype = C.c_int
        L.bh_write_linkage_tsv.argtypes = [vp, C.c_int, C.c_char_p, vp, u64, vp, u64, u32, u32, u64, C.POINTER(u64)]
        L._linkage_ready = True
    return L


def link_rows(ix, file_id, reads, max_mismatches=8):
    """The host twin of link_scan_kernel (linkage.cpp link_rows) over ASCII reads: (rows as [n][32] bytes of bk_link_row in the order
    of the records, (records, placed, unplaced, discordant))."""
    L = _link_lib()
    joined = "\n".join(reads).encode()
    n = C.c_uint64()
    counters = np.zeros(4, np.uint64)
    if L.bh_link_rows(ix.h, file_id, joined, int(max_mismatches), 0, None, C.byref(n), None) != 0:
        raise _host_error(L)
    raw = np.zeros((max(1, n.value), 32), np.uint8)
    if L.bh_link_rows(ix.h, file_id, joined, int(max_mismatches), n.value, raw.ctypes.data, C.byref(n), counters.ctypes.data) != 0:
        raise _host_error(L)
    return raw[:n.value], tuple(int(c) for c in counters)


def link_count(ix, file_id, raw_rows, sites, max_dist=1000):
    """The host twin of link_count_kernel (linkage.cpp link_count): [(site_a, site_b, [16 counters])] in (i, j) order."""
    L = _link_lib()
    raw = np.ascontiguousarray(np.asarray(raw_rows, np.uint8).reshape(-1, 32))
    st = np.ascontiguousarray(np.asarray(sites, np.int64).astype(np.uint32))
    n = C.c_uint64()
    if L.bh_link_count(ix.h, file_id, raw.ctypes.data, len(raw), st.ctypes.data, len(st), int(max_dist), 0, None, C.byref(n)) != 0:
        raise _host_error(L)
    buf = np.zeros((max(1, n.value), 18), np.uint32)
    if L.bh_link_count(ix.h, file_id, raw.ctypes.data, len(raw), st.ctypes.data, len(st), int(max_dist), n.value, buf.ctypes.data, C.byref(n)) != 0:
        raise _host_error(L)
    return [(int(r[0]), int(r[1]), [int(v) for v in r[2:]]) for r in buf[:n.value]]


def write_linkage_tsv(path, ix, file_id, recs, pairs, max_mismatches=8, max_dist=1000, min_reads=1):
    """The --linkage writer (linkage.cpp write_linkage_tsv): recs = [(cell, ref base, alt base)] with 2-bit bases, pairs as
    link_count gives them; returns the lines written."""
    L = _link_lib()
    rc = np.ascontiguousarray(np.asarray(recs, np.int64).reshape(-1, 3).astype(np.uint32))
    buf = np.zeros((max(1, len(pairs)), 18), np.uint32)
    for i, (a, b, c) in enumerate(pairs):
        buf[i, 0], buf[i, 1] = a, b
        buf[i, 2:] = c
    lines = C.c_uint64()
    if L.bh_write_linkage_tsv(ix.h, file_id, path.encode(), rc.ctypes.data, len(rc), buf.ctypes.data, len(pairs), int(max_mismatches), int(max_dist),
                              int(min_reads), C.byref(lines)) != 0:
        raise _host_error(L)
    return lines.value


# ---- --codons: the host twin of the engine's codon count, the BED reader and the writer (codons.cpp) ------------------------------
def _codon_lib():
    L = _caller_lib()
    if not hasattr(L, "_codons_ready"):
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.bh_codon_count.restype = C.c_int
        L.bh_codon_count.argtypes = [vp, C.c_int, vp, u64, vp, u64, u64, vp, C.POINTER(u64)]
        L.bh_codon_bed.restype = C.c_int
        L.bh_codon_bed.argtypes = [vp, C.c_int, C.c_char_p, u64, vp, C.c_char_p, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bh_write_codons_tsv.restype = C.c_int
        L.bh_write_codons_tsv.argtypes = [vp, C.c_int, C.c_char_p, vp, C.c_char_p, u64, vp, u64, u32, u64, C.c_double, C.POINTER(u64)]
        L.bh_translate.restype = C.c_int
        L.bh_translate.argtypes = [C.c_char_p]
        L._codons_ready = True
    return L


def codon_count(ix, file_id, raw_rows, regions):
    """The host twin of the codon kernels (codons.cpp codon_count): counts[codon][16 b0 + 4 b1 + b2] as an (n_codons, 64) uint32 array
    for the regions [(cell0, n_codons), ...], their codons numbered in the order given; raw_rows as link_rows gives them."""
    L = _codon_lib()
    raw = np.ascontiguousarray(np.asarray(raw_rows, np.uint8).reshape(-1, 32))
    rg = np.ascontiguousarray(np.asarray(regions, np.int64).reshape(-1, 2).astype(np.uint32))
    n = int(rg[:, 1].sum())
    out = np.zeros((max(1, n), 64), np.uint32)
    got = C.c_uint64()
    if L.bh_codon_count(ix.h, file_id, raw.ctypes.data, len(raw), rg.ctypes.data, len(rg), n, out.ctypes.data, C.byref(got)) != 0:
        raise _host_error(L)
    assert got.value == n
    return out[:n]


def codon_bed(ix, file_id, path):
    """A --codons BED file read and resolved against genome file file_id (codons.cpp read_codon_bed, resolve_codon_bed):
    [(cell0, n_codons, seq, start, strand, name)] in the file's order; RuntimeError with the file and the line named otherwise."""
    L = _codon_lib()
    n, nl = C.c_uint64(), C.c_uint64()
    if L.bh_codon_bed(ix.h, file_id, path.encode(), 0, None, None, 0, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    genes = np.zeros((max(1, n.value), 5), np.uint32)
    names = C.create_string_buffer(max(1, nl.value))
    if L.bh_codon_bed(ix.h, file_id, path.encode(), n.value, genes.ctypes.data, names, nl.value, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    nm = names.value.decode().split("\n") if n.value else []
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), "-" if r[4] else "+", nm[i]) for i, r in enumerate(genes[:n.value])]


def write_codons_tsv(path, ix, file_id, genes, counts, max_mismatches=8, min_reads=5, min_freq=0.03):
    """The --codons writer (codons.cpp write_codons_tsv): genes as codon_bed gives them, counts (n_codons, 64); returns the lines written."""
    L = _codon_lib()
    g = np.ascontiguousarray(np.array([[c0, nc, seq, start, 1 if strand == "-" else 0] for c0, nc, seq, start, strand, _ in genes], np.int64).reshape(-1, 5).astype(np.uint32))
    names = "\n".join(name for *_, name in genes).encode()
    cnt = np.ascontiguousarray(np.asarray(counts, np.uint32).reshape(-1, 64))
    lines = C.c_uint64()
    if L.bh_write_codons_tsv(ix.h, file_id, path.encode(), g.ctypes.data, names, len(genes), cnt.ctypes.data, len(cnt), int(max_mismatches), int(min_reads),
                             float(min_freq), C.byref(lines)) != 0:
        raise _host_error(L)
    return lines.value


def translate(triplet):
    """The standard code of three letters ACGT (codons.cpp translate)."""
    return chr(_codon_lib().bh_translate(triplet.encode()))


# ---- --haplotypes: the host twin of the engine's haplotype count, the regions and the writer (haplotypes.cpp) ---------------------
def _hap_lib():
    L = _caller_lib()
    if not hasattr(L, "_haps_ready"):
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.bh_hap_count.restype = C.c_int
        L.bh_hap_count.argtypes = [vp, C.c_int, vp, u64, vp, u64, vp, vp, u64, vp, C.POINTER(u64)]
        L.bh_hap_regions.restype = C.c_int
        L.bh_hap_regions.argtypes = [vp, C.c_int, C.c_char_p, u64, u64, u64, vp, C.c_char_p, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bh_write_haplotypes_tsv.restype = C.c_int
        L.bh_write_haplotypes_tsv.argtypes = [vp, C.c_int, C.c_char_p, vp, C.c_char_p, u64, vp, vp, vp, u64, u32, u64, C.c_double, vp]
        L._haps_ready = True
    return L


def _hap_entry_bytes(entries):
    """[(region, count, ((offset, base), ...))] as [n][40] bytes of bk_hap_entry"""
    out = np.zeros((max(1, len(entries)), 40), np.uint8)
    for i, (region, count, mm) in enumerate(entries):
        out[i, :4] = np.frombuffer(int(region).to_bytes(4, "little"), np.uint8)
        out[i, 4:8] = np.frombuffer(int(count).to_bytes(4, "little"), np.uint8)
        out[i, 8] = len(mm)
        for t, (off, b) in enumerate(mm):
            out[i, 16 + 3 * t:19 + 3 * t] = (off & 0xff, off >> 8, b)
    return out


def hap_count(ix, file_id, raw_rows, regions):
    """The host twin of the haplotype kernels (haplotypes.cpp hap_count) for the regions [(cell0, len), ...]: (cover, ref_count,
    entries) -- two uint32 arrays in the regions' order and [(region, count, ((offset, base), ...))] by region, then by list;
    raw_rows as link_rows gives them."""
    from .engine import hap_entries
    L = _hap_lib()
    raw = np.ascontiguousarray(np.asarray(raw_rows, np.uint8).reshape(-1, 32))
    rg = np.ascontiguousarray(np.asarray(regions, np.int64).reshape(-1, 2).astype(np.uint32))
    cover, ref = np.zeros(max(1, len(rg)), np.uint32), np.zeros(max(1, len(rg)), np.uint32)
    got = C.c_uint64()
    if L.bh_hap_count(ix.h, file_id, raw.ctypes.data, len(raw), rg.ctypes.data, len(rg), None, None, 0, None, C.byref(got)) != 0:
        raise _host_error(L)
    buf = np.zeros((max(1, got.value), 40), np.uint8)
    if L.bh_hap_count(ix.h, file_id, raw.ctypes.data, len(raw), rg.ctypes.data, len(rg), cover.ctypes.data, ref.ctypes.data, got.value, buf.ctypes.data, C.byref(got)) != 0:
        raise _host_error(L)
    return cover[:len(rg)], ref[:len(rg)], hap_entries(buf[:got.value])


def hap_regions(ix, file_id, path=None, window=0, step=0):
    """The regions of a --haplotypes BED file (haplotypes.cpp read_hap_bed, resolve_hap_bed) or, with path None, the --hap-window
    tiling (hap_windows) of genome file file_id: [(cell0, len, seq, start, name)] in order; RuntimeError otherwise."""
    L = _hap_lib()
    n, nl = C.c_uint64(), C.c_uint64()
    pth = path.encode() if path is not None else None
    if L.bh_hap_regions(ix.h, file_id, pth, int(window), int(step), 0, None, None, 0, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    wins = np.zeros((max(1, n.value), 4), np.uint32)
    names = C.create_string_buffer(max(1, nl.value))
    if L.bh_hap_regions(ix.h, file_id, pth, int(window), int(step), n.value, wins.ctypes.data, names, nl.value, C.byref(n), C.byref(nl)) != 0:
        raise _host_error(L)
    nm = names.value.decode().split("\n") if n.value else []
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), nm[i]) for i, r in enumerate(wins[:n.value])]


def write_haplotypes_tsv(path, ix, file_id, windows, cover, ref_count, entries, max_mismatches=8, min_reads=5, min_freq=0.03):
    """The --haplotypes writer (haplotypes.cpp write_haplotypes_tsv): windows as hap_regions gives them, the table as hap_count or
    Engine.download_haplotypes gives it; returns (lines written, regions without cover, distinct haplotypes)."""
    L = _hap_lib()
    w = np.ascontiguousarray(np.array([[c0, ln, seq, start] for c0, ln, seq, start, _ in windows], np.int64).reshape(-1, 4).astype(np.uint32))
    names = "\n".join(name for *_, name in windows).encode()
    cv = np.ascontiguousarray(np.resize(np.asarray(cover, np.uint32), max(1, len(windows))))
    rf = np.ascontiguousarray(np.resize(np.asarray(ref_count, np.uint32), max(1, len(windows))))
    en = _hap_entry_bytes(entries)
    stats = (C.c_uint64 * 3)()
    if L.bh_write_haplotypes_tsv(ix.h, file_id, path.encode(), w.ctypes.data, names, len(windows), cv.ctypes.data, rf.ctypes.data, en.ctypes.data, len(entries),
                                 int(max_mismatches), int(min_reads), float(min_freq), stats) != 0:
        raise _host_error(L)
    return tuple(int(v) for v in stats)


# ---- --read-pileup: the host twin of the engine's read pileup and the writer (read_pileup.cpp) ------------------------------------
def _read_pileup_lib():
    L = _caller_lib()
    if not hasattr(L, "_read_pileup_ready"):
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.bh_read_pileup_count.restype = C.c_int
        L.bh_read_pileup_count.argtypes = [vp, C.c_int, vp, u64, u32, u64, vp, C.POINTER(u64)]
        L.bh_write_read_pileup_tsv.restype = C.c_int
        L.bh_write_read_pileup_tsv.argtypes = [vp, C.c_int, C.c_char_p, vp, u64, u32, u32, vp]
        L._read_pileup_ready = True
    return L


def read_pileup_count(ix, file_id, raw_rows, end_dist=10):
    """The host twin of the read-pileup kernels (read_pileup.cpp read_pileup_count): an (n_cells, 12) uint32 array, per position of
    genome file file_id fwd[ACGT], rev[ACGT], near[ACGT]; raw_rows as link_rows gives them."""
    L = _read_pileup_lib()
    raw = np.ascontiguousarray(np.asarray(raw_rows, np.uint8).reshape(-1, 32))
    n = C.c_uint64()
    if L.bh_read_pileup_count(ix.h, file_id, raw.ctypes.data, len(raw), int(end_dist), 0, None, C.byref(n)) != 0:
        raise _host_error(L)
    out = np.zeros((max(1, n.value), 12), np.uint32)
    if L.bh_read_pileup_count(ix.h, file_id, raw.ctypes.data, len(raw), int(end_dist), n.value, out.ctypes.data, C.byref(n)) != 0:
        raise _host_error(L)
    return out[:n.value]


def write_read_pileup_tsv(path, ix, file_id, cells, max_mismatches=8, end_dist=10):
    """The --read-pileup writer (read_pileup.cpp write_read_pileup_tsv): cells (n_cells, 12) as read_pileup_count or
    Engine.download_read_pileup gives them; returns (positions covered, bases)."""
    L = _read_pileup_lib()
    c = np.ascontiguousarray(np.asarray(cells, np.uint32).reshape(-1, 12))
    stats = (C.c_uint64 * 2)()
    if L.bh_write_read_pileup_tsv(ix.h, file_id, path.encode(), c.ctypes.data, len(c), int(max_mismatches), int(end_dist), stats) != 0:
        raise _host_error(L)
    return tuple(int(v) for v in stats)


# ---- --distances: the host twin of the engine's cohort kernels, the clusterer and the three writers (cohort.cpp) ---------------------
def _cohort_lib():
    vp, u64, u32 = _VP, _U64, _U32
    return _bound("_cohort_ready", {
        "bh_cohort_distances": [vp, u64, u64, u64, u64, vp, vp, u32],
        "bh_cohort_clusters": [u64, u64, vp, vp, u64, C.c_double, u64, vp, vp, vp],
        "bh_write_cohort_distances_tsv": [C.c_char_p, C.c_char_p, vp],
        "bh_write_cohort_compared_tsv": [C.c_char_p, C.c_char_p, vp],
        "bh_write_cohort_clusters_tsv": [C.c_char_p, C.c_char_p, vp, vp, u64, C.c_double],
        "bh_cohort_min_compared": [C.c_double, u64],
        "bh_cohort_mst": [vp, u64, u64, u32, u32, vp, vp, vp],
        "bh_cohort_root_forest": [u64, vp, u64, vp, vp, vp, vp, vp, vp],
        "bh_write_cohort_mst_tsv": [C.c_char_p, C.c_char_p, vp, u64, vp, C.c_double, u32]})


def cohort_min_compared(min_breadth, positions):
    """The smallest integer c with float(c) >= min_breadth * float(positions) (cohort.cpp cohort_min_compared): --mst-min-breadth as a count."""
    L = _cohort_lib()
    L.bh_cohort_min_compared.restype = C.c_uint32
    return int(L.bh_cohort_min_compared(float(min_breadth), int(positions)))


def cohort_mst(letters, min_compared=0, threads=4):
    """The host twin of bk_cohort_mst (cohort.cpp cohort_mst_host: Prim per component): (edges, nearest) of an (n_samples, positions)
    uint8 array of letters -- an (E, 4) uint32 array of lo, hi, diff, compared, ascending in the edge order, and an (n, 3) uint32
    array of sample (0xffffffff: none), diff, compared."""
    L = _cohort_lib()
    a = np.ascontiguousarray(letters, np.uint8)
    n, positions = a.shape
    edges = np.zeros((max(1, n), 4), np.uint32)
    nearest = np.zeros((max(1, n), 3), np.uint32)
    n_edges = C.c_uint64(0)
    if L.bh_cohort_mst(a.ctypes.data, n, positions, int(min_compared), int(threads), edges.ctypes.data, C.addressof(n_edges), nearest.ctypes.data) != 0:
        raise _host_error(L)
    return edges[:int(n_edges.value)], nearest[:n]


def cohort_root_forest(n, edges):
    """cohort.cpp root_forest: (parent, diff, compared, component, size, n_components, largest, longest) of a forest's (E, 4) edges; a
    root's parent is 0xffffffff."""
    L = _cohort_lib()
    e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 4)
    out = [np.zeros(max(1, n), np.uint32) for _ in range(5)]
    stats = np.zeros(3, np.uint32)
    if L.bh_cohort_root_forest(int(n), e.ctypes.data, len(e), *[o.ctypes.data for o in out], stats.ctypes.data) != 0:
        raise _host_error(L)
    return tuple(o[:n] for o in out) + tuple(int(v) for v in stats)


def write_cohort_mst_tsv(path, names, edges, nearest, min_breadth, min_compared):
    """The --mst writer (cohort.cpp root_forest and write_cohort_mst_tsv): OUT/<genome>.mst.tsv of a forest's edges and the nearest neighbours."""
    L = _cohort_lib()
    e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 4)
    nr = np.ascontiguousarray(nearest, np.uint32).reshape(-1, 3)
    if len(nr) != len(names):
        raise ValueError("write_cohort_mst_tsv: one nearest neighbour per sample")
    if L.bh_write_cohort_mst_tsv(path.encode(), "\n".join(names).encode(), e.ctypes.data, len(e), nr.ctypes.data, float(min_breadth), int(min_compared)) != 0:
        raise _host_error(L)


def cohort_distances(letters, row0=0, n_rows=None, threads=4):
    """The host twin of the cohort kernels (cohort.cpp cohort_distances_host): (diff, compared) of the rows [row0, row0 + n_rows) of an
    (n_samples, positions) uint8 array of letters against all of its rows, two (n_rows, n_samples) uint32 arrays."""
    L = _cohort_lib()
    a = np.ascontiguousarray(letters, np.uint8)
    n, positions = a.shape
    n_rows = n - row0 if n_rows is None else n_rows
    diff = np.zeros((max(1, n_rows), max(1, n)), np.uint32)
    compared = np.zeros_like(diff)
    if L.bh_cohort_distances(a.ctypes.data, n, positions, int(row0), int(n_rows), diff.ctypes.data, compared.ctypes.data, int(threads)) != 0:
        raise _host_error(L)
    return diff[:n_rows, :n], compared[:n_rows, :n]


def cohort_clusters(diff, compared, positions, threshold, min_breadth=0.9, block_rows=0):
    """The --clusters clusterer (cohort.cpp CohortClusterer) fed the two (n, n) matrices in blocks of block_rows rows (0: at once):
    (cluster numbers, cluster sizes, number of clusters, size of the largest)."""
    L = _cohort_lib()
    d = np.ascontiguousarray(diff, np.uint32)
    c = np.ascontiguousarray(compared, np.uint32)
    n = d.shape[0]
    cluster = np.zeros(max(1, n), np.uint32)
    size = np.zeros(max(1, n), np.uint32)
    stats = np.zeros(2, np.uint32)
    if L.bh_cohort_clusters(n, int(positions), d.ctypes.data, c.ctypes.data, int(threshold), float(min_breadth), int(block_rows),
                            cluster.ctypes.data, size.ctypes.data, stats.ctypes.data) != 0:
        raise _host_error(L)
    return cluster[:n], size[:n], int(stats[0]), int(stats[1])


def write_cohort_matrix_tsv(path, names, matrix, compared=False):
    """The --distances writers (cohort.cpp): OUT/<genome>.distances.tsv, or .compared.tsv with compared=True, of an (n, n) matrix."""
    L = _cohort_lib()
    m = np.ascontiguousarray(matrix, np.uint32)
    fn = L.bh_write_cohort_compared_tsv if compared else L.bh_write_cohort_distances_tsv
    if fn(path.encode(), "\n".join(names).encode(), m.ctypes.data) != 0:
        raise _host_error(L)


def write_cohort_clusters_tsv(path, names, cluster, size, threshold, min_breadth=0.9):
    """The --clusters writer (cohort.cpp write_cohort_clusters_tsv)."""
    L = _cohort_lib()
    cl = np.ascontiguousarray(cluster, np.uint32)
    sz = np.ascontiguousarray(size, np.uint32)
    if L.bh_write_cohort_clusters_tsv(path.encode(), "\n".join(names).encode(), cl.ctypes.data, sz.ctypes.data, int(threshold), float(min_breadth)) != 0:
        raise _host_error(L)


# ---- --contamination: the host twins, the scanner and the three writers (cohort.cpp) ------------------------------------------------
def _contamination_lib():
    vp, u64, u32 = _VP, _U64, _U32
    return _bound("_contamination_ready", {
        "bh_minor_mask": [vp, vp, u64, u64, C.c_double, vp, vp],
        "bh_cohort_explained": [vp, vp, u64, u64, u64, u64, vp, vp, u32],
        "bh_contamination_scan": [u64, vp, vp, vp, u32, C.c_double, u64, vp, u64, vp, vp, vp, vp],
        "bh_write_cohort_explained_tsv": [C.c_char_p, C.c_char_p, vp],
        "bh_write_contamination_tsv": [C.c_int, C.c_char_p, C.c_char_p, vp, vp, vp, vp, u64, C.c_double, u32, C.c_double, u64]})


def minor_mask(fwd, rev, min_reads=10, min_freq=0.03):
    """The host twin of bk_sample_minor_alleles (cohort.cpp minor_mask_host) over the positions of two (positions * 4) uint64 depth
    arrays: (masks as a uint8 array, (positions, mixed, present))."""
    L = _contamination_lib()
    f = np.ascontiguousarray(fwd, np.uint64).reshape(-1)
    r = np.ascontiguousarray(rev, np.uint64).reshape(-1)
    if len(f) != len(r) or len(f) % 4:
        raise ValueError("minor_mask: four counts a position on either strand")
    positions = len(f) // 4
    masks = np.zeros(max(1, positions), np.uint8)
    tallies = np.zeros(3, np.uint64)
    if L.bh_minor_mask(f.ctypes.data, r.ctypes.data, positions, int(min_reads), float(min_freq), masks.ctypes.data, tallies.ctypes.data) != 0:
        raise _host_error(L)
    return masks[:positions], tuple(int(v) for v in tallies)


def cohort_explained(letters, masks, row0=0, n_rows=None, threads=4):
    """The host twin of bk_cohort_set_minor and bk_cohort_explained (cohort.cpp cohort_explained_host): (explained, minor_sites) of the
    rows [row0, row0 + n_rows) of two (n_samples, positions) uint8 arrays -- an (n_rows, n_samples) and an (n_rows,) uint32 array."""
    L = _contamination_lib()
    a = np.ascontiguousarray(letters, np.uint8)
    m = np.ascontiguousarray(masks, np.uint8)
    if a.shape != m.shape or a.ndim != 2:
        raise ValueError("cohort_explained: a mask per letter")
    n, positions = a.shape
    n_rows = n - row0 if n_rows is None else n_rows
    explained = np.zeros((max(1, n_rows), max(1, n)), np.uint32)
    sites = np.zeros(max(1, n_rows), np.uint32)
    if L.bh_cohort_explained(a.ctypes.data, m.ctypes.data, n, positions, int(row0), int(n_rows), explained.ctypes.data, sites.ctypes.data, int(threads)) != 0:
        raise _host_error(L)
    return explained[:n_rows, :n], sites[:n_rows]


def _three_matrices(diff, compared, explained):
    d, c, x = (np.ascontiguousarray(v, np.uint32) for v in (diff, compared, explained))
    if not (d.ndim == 2 and d.shape[0] == d.shape[1] and d.shape == c.shape == x.shape):
        raise ValueError("three (n, n) matrices")
    return d, c, x


def contamination_scan(diff, compared, explained, min_sites=3, min_share=0.75, block_rows=0):
    """The --contamination scanner (cohort.cpp ContaminationScanner) fed the three (n, n) matrices in blocks of block_rows rows (0: at
    once): (flagged, best, counts, recipients, largest) -- flagged an (F, 5) uint32 array of recipient, source, diff, compared,
    explained, ordered by (recipient, source); best an (n, 3) array of source (0xffffffff: none), explained, diff; counts the sources
    every sample is flagged for."""
    L = _contamination_lib()
    d, c, x = _three_matrices(diff, compared, explained)
    n = d.shape[0]
    cap = max(1, n * n)
    flagged = np.zeros((cap, 5), np.uint32)
    best = np.zeros((max(1, n), 3), np.uint32)
    counts = np.zeros(max(1, n), np.uint32)
    stats = np.zeros(2, np.uint32)
    n_flagged = C.c_uint64(0)
    if L.bh_contamination_scan(n, d.ctypes.data, c.ctypes.data, x.ctypes.data, int(min_sites), float(min_share), int(block_rows), flagged.ctypes.data, cap,
                               C.addressof(n_flagged), best.ctypes.data, counts.ctypes.data, stats.ctypes.data) != 0:
        raise _host_error(L)
    return flagged[:int(n_flagged.value)], best[:n], counts[:n], int(stats[0]), int(stats[1])


def write_cohort_explained_tsv(path, names, explained):
    """The --contamination matrix writer (cohort.cpp): OUT/<genome>.explained.tsv of an (n, n) matrix."""
    L = _contamination_lib()
    m = np.ascontiguousarray(explained, np.uint32)
    if L.bh_write_cohort_explained_tsv(path.encode(), "\n".join(names).encode(), m.ctypes.data) != 0:
        raise _host_error(L)


def write_contamination_tsv(path, names, diff, compared, explained, minor_sites, minor_min_reads=10, minor_min_freq=0.03, min_sites=3, min_share=0.75,
                            mixture=False, block_rows=0):
    """The --contamination writers (cohort.cpp): OUT/<genome>.contamination.tsv, or .mixture.tsv with mixture=True, of the scanner's
    result over the three (n, n) matrices."""
    L = _contamination_lib()
    d, c, x = _three_matrices(diff, compared, explained)
    ms = np.ascontiguousarray(minor_sites, np.uint32)
    if len(ms) != len(names) or d.shape[0] != len(names):
        raise ValueError("write_contamination_tsv: one row and one minor_sites per sample")
    if L.bh_write_contamination_tsv(1 if mixture else 0, path.encode(), "\n".join(names).encode(), d.ctypes.data, c.ctypes.data, x.ctypes.data, ms.ctypes.data,
                                    int(minor_min_reads), float(minor_min_freq), int(min_sites), float(min_share), int(block_rows)) != 0:
        raise _host_error(L)
