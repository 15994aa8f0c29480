"""Python mirror of the C ABI (include/bronko_hip.h): same call order, same argument meaning, same errors.

    eng = Engine(k, bucket_ids, bucket_off, entries, files, Params(...))   # = bk_engine_create
    eng.sample_begin()                                                      # = initialize_output_maps
    eng.push_reads(mate, words, lens)                                       # = reads of one mate file
    res = eng.sample_finish(n_mates)                                        # = KMC thresholds + map_kmers

A non-zero status raises BronkoError with bk_last_error(); the reference's convention for the same
conditions is `error!(..); exit(1)`.
"""
import ctypes as C

import numpy as np

from . import _ffi

BUCKET_INFO_DTYPE = np.dtype({"names": ["file_id", "seq_id", "location", "idx", "canonical"],
                              "formats": [np.uint16, np.uint8, np.uint32, np.uint8, np.uint8],
                              "offsets": [0, 2, 4, 8, 9], "itemsize": 12})


class BronkoError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("bronko_hip status %d: %s" % (status, msg))
        self.status = status


def lib_path():
    return _ffi.LIB_PATH


def _check(rc, L=None):
    if rc != 0:
        raise BronkoError(rc, (L or _ffi.load()).bk_last_error().decode(errors="replace"))


def Params(n_fixed=2, use_full_kmer=False, ci=3, cs=1000000, cx=1000000000, device=0, full_kmer_stats=False,
           kmer_table_log2=None, pileup_selected_only=False):
    p = _ffi.Params()
    _ffi.load().bk_params_default(C.byref(p))
    p.n_fixed, p.use_full_kmer, p.ci, p.cs, p.cx, p.device = n_fixed, int(use_full_kmer), ci, cs, cx, device
    p.full_kmer_stats = int(full_kmer_stats)
    p.pileup_selected_only = int(pileup_selected_only)
    if kmer_table_log2 is not None:
        p.kmer_table_log2 = kmer_table_log2
    return p


def pack_reads(reads, k, stride_words=None):
    """K0 (bk_pack_reads): list of ASCII reads -> (words u32[n][stride], lens u16[n]) fixed-stride 2-bit records."""
    L = _ffi.load()
    reads = [bytes(r) for r in reads]
    if stride_words is None:
        longest = max([len(r) for r in reads] + [k])
        stride_words = min((longest + 15) // 16, 4095)
    flat = np.frombuffer(b"".join(reads), np.uint8) if reads else np.zeros(0, np.uint8)
    flat = np.ascontiguousarray(flat) if len(flat) else np.zeros(1, np.uint8)
    off = np.zeros(len(reads) + 1, np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads])
    n = L.bk_pack_reads_flat(flat.ctypes.data, off.ctypes.data, len(reads), k, stride_words, None, None, 0)
    words = np.zeros((max(n, 1), stride_words), np.uint32)
    lens = np.zeros(max(n, 1), np.uint16)
    L.bk_pack_reads_flat(flat.ctypes.data, off.ctypes.data, len(reads), k, stride_words, words.ctypes.data,
                         lens.ctypes.data, n)
    return words[:n], lens[:n]


def pack_reads_ends(reads, k, stride_words=None):
    """bk_pack_reads_flat_ends: pack_reads plus the records' end flags u8[n] (bit 0: the record starts its read, bit 1: ends it)."""
    L = _ffi.load()
    reads = [bytes(r) for r in reads]
    if stride_words is None:
        longest = max([len(r) for r in reads] + [k])
        stride_words = min((longest + 15) // 16, 4095)
    flat = np.frombuffer(b"".join(reads), np.uint8) if reads else np.zeros(0, np.uint8)
    flat = np.ascontiguousarray(flat) if len(flat) else np.zeros(1, np.uint8)
    off = np.zeros(len(reads) + 1, np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads])
    n = L.bk_pack_reads_flat_ends(flat.ctypes.data, off.ctypes.data, len(reads), k, stride_words, None, None, None, 0)
    words = np.zeros((max(n, 1), stride_words), np.uint32)
    lens = np.zeros(max(n, 1), np.uint16)
    ends = np.zeros(max(n, 1), np.uint8)
    L.bk_pack_reads_flat_ends(flat.ctypes.data, off.ctypes.data, len(reads), k, stride_words, words.ctypes.data, lens.ctypes.data,
                              ends.ctypes.data, n)
    return words[:n], lens[:n], ends[:n]


def build_index_device(k, files, device=0):
    """bk_build_index: build_indexes (build.rs:145-231) on the GPU.  files = [(file_name, [(seq_name, seq_bytes), ...]), ...];
    returns (bucket_ids u64[n], bucket_off u64[n + 1], entries BucketInfo[m]) -- what Engine() takes."""
    L = _ffi.load()
    n_seqs = np.array([len(f[1]) for f in files] + [0], np.int32)
    seqs = [bytes(s[1]) for f in files for s in f[1]]
    seq_lens = np.array([len(s) for s in seqs] + [0], np.uint64)
    bufs = [C.create_string_buffer(s, max(len(s), 1)) for s in seqs]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.addressof(b) for b in bufs])
    out = _ffi.BuiltIndex()
    rc = L.bk_build_index(k, len(files), n_seqs.ctypes.data, seq_lens.ctypes.data, C.addressof(ptrs), device, C.byref(out))
    if rc != 0:
        raise BronkoError(rc, L.bk_build_last_error().decode(errors="replace"))
    try:
        nb, ne = out.n_buckets, out.n_entries
        ids = np.ctypeslib.as_array(C.cast(out.bucket_ids, C.POINTER(C.c_uint64)), shape=(nb,)).copy() if nb else np.zeros(0, np.uint64)
        off = np.ctypeslib.as_array(C.cast(out.bucket_off, C.POINTER(C.c_uint64)), shape=(nb + 1,)).copy()
        ent = (np.ctypeslib.as_array(C.cast(out.entries, C.POINTER(C.c_uint8)), shape=(ne * 12,)).copy().view(BUCKET_INFO_DTYPE)
               if ne else np.zeros(0, BUCKET_INFO_DTYPE))
    finally:
        L.bk_built_index_free(C.byref(out))
    return ids, off, ent


class SampleResult:
    """Outputs of one sample: the four OutputData arrays (call.rs:1235-1239,1451-1454) + map_kmers' stats."""

    def __init__(self, n_mates, n_files, total_cells):
        n = total_cells * 4
        self.fwd_depth = np.zeros(n, np.uint64)
        self.rev_depth = np.zeros(n, np.uint64)
        self.fwd_nk = np.zeros(n, np.uint64)
        self.rev_nk = np.zeros(n, np.uint64)
        self.stats = np.zeros((n_mates, n_files, 3), np.uint64)
        self.present = np.zeros((n_mates, n_files), np.uint8)
        self.kmer_stats = np.zeros((n_mates, 4), np.uint64)

    def arrays(self):
        return self.fwd_depth, self.rev_depth, self.fwd_nk, self.rev_nk


def device_memory(device=0):
    """(free, total) bytes of a device (bk_device_memory): what the CLI sizes its number of ingest lanes by."""
    L = _ffi.load()
    f, t = C.c_uint64(), C.c_uint64()
    _check(L.bk_device_memory(device, C.byref(f), C.byref(t)), L)
    return f.value, t.value


class Engine:
    def __init__(self, k, bucket_ids, bucket_off, entries, files, params=None):
        """files: [(file_name, [(seq_name, seq_bytes), ...]), ...] = ViralMetadata (build.rs:46-50)"""
        L = _ffi.load()
        self._L = L
        self.h = None
        params = params or Params()
        ids = np.ascontiguousarray(bucket_ids, np.uint64)
        off = np.ascontiguousarray(bucket_off, np.uint64)
        ent = np.ascontiguousarray(entries)
        if ent.dtype != BUCKET_INFO_DTYPE:
            raise TypeError("entries must have the 12-byte BucketInfo dtype")
        n_seqs = np.array([len(f[1]) for f in files] + [0], np.int32)
        seqs = [bytes(s[1]) for f in files for s in f[1]]
        seq_lens = np.array([len(s) for s in seqs] + [0], np.uint64)
        bufs = [C.create_string_buffer(s, max(len(s), 1)) for s in seqs]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.addressof(b) for b in bufs])
        d = _ffi.IndexDesc(k, len(ids), ids.ctypes.data, off.ctypes.data, ent.ctypes.data, len(ent), len(files),
                           n_seqs.ctypes.data, seq_lens.ctypes.data, C.addressof(ptrs))
        h = C.c_void_p()
        _check(L.bk_engine_create(C.byref(d), C.byref(params), C.byref(h)), L)
        self.h = h
        self.k = k
        self.params = params
        self.n_files = L.bk_n_files(h)
        self.total_cells = L.bk_total_cells(h)
        self.n_slots = L.bk_n_slots(h)
        self.counter_len = L.bk_counter_len(h)

    def fork(self, params=None):
        """A second engine on the same device tables with its own counter planes, outputs and stream (bk_engine_fork):
        alternate independent samples over the two so that one's scan overlaps the other's finalize.  params: the fork's own
        ci / cs / cx / pileup_selected_only (bk_engine_fork_params; what shapes the tables must equal the parent's)."""
        h = C.c_void_p()
        if params is None:
            _check(self._L.bk_engine_fork(self.h, C.byref(h)), self._L)
        else:
            _check(self._L.bk_engine_fork_params(self.h, C.byref(params), C.byref(h)), self._L)
        e = object.__new__(Engine)
        e._L, e.h, e.k, e.params = self._L, h, self.k, params if params is not None else self.params
        e.n_files, e.total_cells, e.n_slots, e.counter_len = self.n_files, self.total_cells, self.n_slots, self.counter_len
        e._parent = self   # the parent's tables must outlive the fork
        return e

    def close(self):
        if self.h:
            self._L.bk_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(self._L.bk_engine_set_stream(self.h, C.c_void_p(stream_ptr)), self._L)

    def stream_ptr(self):
        """hipStream_t (as int) the engine launches on -- wrap it (torch.cuda.ExternalStream) to order other work with it."""
        return int(self._L.bk_engine_get_stream(self.h) or 0)

    def sample_begin(self):
        _check(self._L.bk_sample_begin(self.h), self._L)

    def push_reads(self, mate, words, lens):
        words = np.ascontiguousarray(words, np.uint32)
        lens = np.ascontiguousarray(lens, np.uint16)
        if len(lens) == 0:
            return
        assert words.ndim == 2 and words.shape[0] == len(lens)
        _check(self._L.bk_push_reads_packed(self.h, mate, words.ctypes.data, words.shape[1], lens.ctypes.data, len(lens)), self._L)

    def primers_set(self, primers, max_mismatches=1):
        """bk_primers_set: primers (bytes, 5'->3') trimmed from the ends of every read pushed from now on; [] clears them."""
        primers = [bytes(p) for p in primers]
        bufs = [C.create_string_buffer(p, max(len(p), 1)) for p in primers]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.addressof(b) for b in bufs])
        lens = np.array([len(p) for p in primers] + [0], np.uint32)
        _check(self._L.bk_primers_set(self.h, C.addressof(ptrs), lens.ctypes.data, len(primers), max_mismatches), self._L)

    def primer_stats(self, mate):
        """bk_primer_stats: [reads trimmed at 5', reads trimmed at 3', bases masked] of the sample just finalized."""
        out = np.zeros(3, np.uint64)
        _check(self._L.bk_primer_stats(self.h, mate, out.ctypes.data), self._L)
        return out.tolist()

    def adapters_set(self, adapters, min_overlap=5, max_error_rate=0.1):
        """bk_adapters_set: 3' adapters (bytes, 5'->3' as they appear in a read) cut off every read pushed from now on; [] clears them."""
        adapters = [bytes(a) for a in adapters]
        bufs = [C.create_string_buffer(a, max(len(a), 1)) for a in adapters]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.addressof(b) for b in bufs])
        lens = np.array([len(a) for a in adapters] + [0], np.uint32)
        _check(self._L.bk_adapters_set(self.h, C.addressof(ptrs), lens.ctypes.data, len(adapters), min_overlap, max_error_rate), self._L)

    def adapter_stats(self, mate):
        """bk_adapter_stats: [reads cut, bases removed] of the sample just finalized."""
        out = np.zeros(2, np.uint64)
        _check(self._L.bk_adapter_stats(self.h, mate, out.ctypes.data), self._L)
        return out.tolist()

    def push_reads_ends(self, mate, words, lens, ends):
        """bk_push_reads_packed_ends: packed records with their end flags (pack_reads_ends)."""
        words = np.ascontiguousarray(words, np.uint32)
        lens = np.ascontiguousarray(lens, np.uint16)
        ends = np.ascontiguousarray(ends, np.uint8)
        if len(lens) == 0:
            return
        assert words.ndim == 2 and words.shape[0] == len(lens) == len(ends)
        _check(self._L.bk_push_reads_packed_ends(self.h, mate, words.ctypes.data, words.shape[1], lens.ctypes.data, ends.ctypes.data,
                                                 len(lens)), self._L)

    def push_reads_ends_device(self, mate, d_words_ptr, stride_words, d_lens_ptr, d_ends_ptr, n_records):
        _check(self._L.bk_push_reads_packed_ends_device(self.h, mate, C.c_void_p(d_words_ptr), stride_words, C.c_void_p(d_lens_ptr),
                                                        C.c_void_p(d_ends_ptr), n_records), self._L)

    def push_reads_ascii(self, mate, reads, quals=None, min_qual=0):
        """bk_push_reads_ascii: list of ASCII reads, packed on the GPU, asynchronous.  With quals (one quality line per read, same
        lengths) and min_qual > 0: bk_push_reads_ascii_qual -- a base whose quality byte is below '!' + min_qual counts as N."""
        reads = [bytes(r) for r in reads]
        if not reads:
            return
        flat = np.frombuffer(b"".join(reads), np.uint8)
        flat = np.ascontiguousarray(flat) if len(flat) else np.zeros(1, np.uint8)
        off = np.zeros(len(reads) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in reads])
        if quals is None and min_qual == 0:
            _check(self._L.bk_push_reads_ascii(self.h, mate, flat.ctypes.data, off.ctypes.data, len(reads)), self._L)
            return
        qflat = None
        if quals is not None:
            quals = [bytes(q) for q in quals]
            if len(quals) != len(reads) or any(len(q) != len(r) for q, r in zip(quals, reads)):
                raise ValueError("push_reads_ascii: every quality line must be as long as its read")
            qflat = np.frombuffer(b"".join(quals), np.uint8)
            qflat = np.ascontiguousarray(qflat) if len(qflat) else np.zeros(1, np.uint8)
        _check(self._L.bk_push_reads_ascii_qual(self.h, mate, flat.ctypes.data, None if qflat is None else qflat.ctypes.data, off.ctypes.data,
                                                len(reads), min_qual), self._L)

    def push_reads_ascii_device(self, mate, d_bases_ptr, d_offsets_ptr, n_reads, total_bases, longest_read, quals=None, min_qual=0):
        """bk_push_reads_ascii_device: sequence lines resident in device memory, packed (K0) and scanned on the engine's stream.
        quals: device pointer of the quality lines (same offsets; bk_push_reads_ascii_qual_device with min_qual)."""
        if quals is None and min_qual == 0:
            _check(self._L.bk_push_reads_ascii_device(self.h, mate, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), n_reads, total_bases,
                                                      longest_read), self._L)
            return
        _check(self._L.bk_push_reads_ascii_qual_device(self.h, mate, C.c_void_p(d_bases_ptr), C.c_void_p(quals), C.c_void_p(d_offsets_ptr),
                                                       n_reads, total_bases, longest_read, min_qual), self._L)

    def push_reads_device(self, mate, d_words_ptr, stride_words, d_lens_ptr, n_records):
        _check(self._L.bk_push_reads_packed_device(self.h, mate, C.c_void_p(d_words_ptr), stride_words,
                                                   C.c_void_p(d_lens_ptr), n_records), self._L)

    def counters_ptr(self, mate):
        p = C.c_void_p()
        _check(self._L.bk_counters_device_ptr(self.h, mate, C.byref(p)), self._L)
        return p.value

    def pileup_ptr(self):
        p = C.c_void_p()
        _check(self._L.bk_pileup_device_ptr(self.h, C.byref(p)), self._L)
        return p.value

    def sample_finalize(self, n_mates=1):
        _check(self._L.bk_sample_finalize(self.h, n_mates), self._L)

    def sample_finalize_shard(self, n_mates, shard, n_shards):
        """Map only the shard-th of n_shards equal parts of each counter plane (include/bronko_hip.h)."""
        _check(self._L.bk_sample_finalize_shard(self.h, n_mates, shard, n_shards), self._L)

    def shard_measure(self, mate):
        """Device pointer of two u64: the largest E count and the largest |V element| of this rank's plane (asynchronous; the
        host all-reduces them with MAX and picks the transport width: include/bronko_hip.h)."""
        p = C.c_void_p()
        _check(self._L.bk_shard_measure(self.h, mate, C.byref(p)), self._L)
        return p.value

    def shard_transport(self, mate, n_shards, width):
        """Pack the plane for the reduce-scatter: (send pointer, bytes per part, receive pointer); width 16 / 32 / 64 bits."""
        s, r, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(self._L.bk_shard_transport(self.h, mate, n_shards, width, C.byref(s), C.byref(n), C.byref(r)), self._L)
        return s.value, n.value, r.value

    def shard_received(self, mate, shard, n_shards, width):
        _check(self._L.bk_shard_received(self.h, mate, shard, n_shards, width), self._L)

    def transport_overflow(self):
        """True when some sample since the last call met a counter too large for the width its plane was exchanged at."""
        f = C.c_int(0)
        _check(self._L.bk_transport_overflow(self.h, C.byref(f)), self._L)
        return bool(f.value)

    def kmer_table_partition(self, n_parts):
        """full_kmer_stats under a sharded finalize: (device pointer of keys u64, of counts u32, offsets[n_parts + 1]) -- the
        statistics table's entries grouped by owner rank.  Synchronises."""
        k, c = C.c_void_p(), C.c_void_p()
        off = (C.c_uint64 * (n_parts + 1))()
        _check(self._L.bk_kmer_table_partition(self.h, n_parts, C.byref(k), C.byref(c), off), self._L)
        return k.value, c.value, list(off)

    def kmer_table_replace(self, keys_ptr, counts_ptr, n):
        """... and the table rebuilt from the entries this rank owns (device pointers; equal keys add up)."""
        _check(self._L.bk_kmer_table_replace(self.h, keys_ptr, counts_ptr, n), self._L)

    def kmer_dump_enable(self, log2=26):
        """Count every strand-specific k-mer of the samples from the next sample_begin on (bk_kmer_dump_enable; 0 disables):
        the KMC -b -ci -cs -cx table that `bronko call --keep-kmer-info` writes out."""
        _check(self._L.bk_kmer_dump_enable(self.h, log2), self._L)

    def kmer_dump_size(self, mate=0):
        """(n_kept, n_distinct) of a finalized mate file (2**64 - 1 for both if the table overflowed)."""
        kept, distinct = C.c_uint64(), C.c_uint64()
        _check(self._L.bk_kmer_dump_size(self.h, mate, C.byref(kept), C.byref(distinct)), self._L)
        return kept.value, distinct.value

    def kmer_dump(self, mate=0):
        """(kmers u64[], counts u64[]) of a finalized mate file: the kept k-mers ascending (MSB-first 2-bit codes), min(count, cs)."""
        kept, _ = self.kmer_dump_size(mate)
        km = np.zeros(max(kept, 1), np.uint64)
        ct = np.zeros(max(kept, 1), np.uint64)
        _check(self._L.bk_kmer_dump_download(self.h, mate, km.ctypes.data, ct.ctypes.data, kept), self._L)
        return km[:kept], ct[:kept]

    @property
    def full_kmer_stats(self):
        return bool(self.params.full_kmer_stats)

    def shard_sums(self):
        """(device pointer, u64 length) of the small additive results of sample_finalize_shard."""
        p, n = C.c_void_p(), C.c_uint64()
        _check(self._L.bk_shard_sums_device_ptr(self.h, C.byref(p), C.byref(n)), self._L)
        return p.value, n.value

    def sample_merge_shards(self):
        _check(self._L.bk_sample_merge_shards(self.h), self._L)

    def sample_download(self, n_mates=1, arrays=True):
        r = SampleResult(n_mates, self.n_files, self.total_cells)
        a = [x.ctypes.data if arrays else None for x in (r.fwd_depth, r.rev_depth, r.fwd_nk, r.rev_nk)]
        _check(self._L.bk_sample_download(self.h, n_mates, a[0], a[1], a[2], a[3], r.stats.ctypes.data,
                                          r.present.ctypes.data, r.kmer_stats.ctypes.data), self._L)
        return r

    def sample_finish(self, n_mates=1):
        self.sample_finalize(n_mates)
        return self.sample_download(n_mates)

    def call_params(self, **kw):
        """bk_call_params with the reference's defaults (cli.rs:92-135), k = the engine's; keyword overrides."""
        p = _ffi.CallParams()
        self._L.bk_call_params_default(C.byref(p))
        p.k = self.k
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    def sample_call(self, n_mates=1, params=None):
        """Reference selection + baseline noise + variant calls on the device for the sample just finalized (asynchronous)."""
        _check(self._L.bk_sample_call(self.h, n_mates, C.byref(params or self.call_params())), self._L)

    def download_calls(self):
        """(summary, records) of sample_call: records sorted by (sequence, position, alternative base)."""
        summ = _ffi.CallSummary()
        _check(self._L.bk_sample_download_calls(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many records there are)
        cap = max(1, int(summ.n_records))
        recs = (_ffi.CallRecord * cap)()
        _check(self._L.bk_sample_download_calls(self.h, C.byref(summ), recs, cap), self._L)
        return summ, [recs[i] for i in range(min(summ.n_records, cap))]

    def download_noise(self):
        """Noise.max per position of the genome sample_call selected (diagnostic; call.rs:953-962)."""
        n = C.c_uint64(0)
        out = np.zeros(max(1, self.total_cells), np.float64)
        _check(self._L.bk_sample_download_noise(self.h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), self._L)
        return out[:n.value]

    def consensus_params(self, **kw):
        """bk_consensus_params with the defaults (min_depth 10, min_freq 0.5); keyword overrides."""
        p = _ffi.ConsensusParams()
        self._L.bk_consensus_params_default(C.byref(p))
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    def sample_consensus(self, params=None):
        """One consensus letter per position of the genome sample_call selected, on the device (asynchronous)."""
        _check(self._L.bk_sample_consensus(self.h, C.byref(params or self.consensus_params())), self._L)

    def download_consensus(self, cap=None):
        """(summary, letters as bytes) of sample_consensus: min(cap, summary.positions) letters, all of them by default."""
        summ = _ffi.ConsensusSummary()
        if cap is None:
            _check(self._L.bk_sample_download_consensus(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many letters there are)
            cap = int(summ.positions)
        buf = np.zeros(max(1, cap), np.uint8)
        _check(self._L.bk_sample_download_consensus(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, buf[:min(cap, int(summ.positions))].tobytes()

    def minor_params(self, **kw):
        """bk_minor_params with the defaults (min_reads 10, min_freq 0.03); keyword overrides."""
        p = _ffi.MinorParams()
        self._L.bk_minor_params_default(C.byref(p))
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    def sample_minor_alleles(self, params=None):
        """The present mask of every position of the genome sample_call selected, on the device (asynchronous)."""
        _check(self._L.bk_sample_minor_alleles(self.h, C.byref(params or self.minor_params())), self._L)

    def download_minor_alleles(self, cap=None):
        """(summary, masks as a uint8 array) of sample_minor_alleles: min(cap, summary.positions) bytes, all of them by default."""
        summ = _ffi.MinorSummary()
        if cap is None:
            _check(self._L.bk_sample_download_minor_alleles(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many bytes there are)
            cap = int(summ.positions)
        buf = np.zeros(max(1, cap), np.uint8)
        _check(self._L.bk_sample_download_minor_alleles(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, buf[:min(cap, int(summ.positions))]

    def _download_events(self, download, summ, cap, dtype, columns=None):
        """What the six download_x of the event passes do alike: (summary, min(cap, summary.reported) rows of `dtype`, `columns` wide) --
        all rows when cap is None, by asking for the summary first."""
        if cap is None:
            _check(download(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many rows there are)
            cap = int(summ.reported)
        buf = np.zeros(max(1, cap) if columns is None else (max(1, cap), columns), dtype)
        _check(download(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, buf[:min(cap, int(summ.reported))]

    def _download_event_span(self, download):
        """... and the six download_x_span: the prefix-summed span array of all cells."""
        span = np.zeros(max(1, self.total_cells), np.uint32)
        _check(download(self.h, span.ctypes.data_as(C.c_void_p), self.total_cells), self._L)
        return span[:self.total_cells]

    def indels_enable(self, max_len=32, max_mismatches=2, table_log2=16):
        """bk_indels_enable: indel_scan_kernel runs behind every scan of the samples that begin from now on; max_len=None disables."""
        cfg = None if max_len is None else C.byref(_ffi.IndelConfig(int(max_len), int(max_mismatches), int(table_log2)))
        _check(self._L.bk_indels_enable(self.h, cfg), self._L)

    def sample_indels(self, min_reads=5, min_af_ppm=30000):
        """bk_sample_indels: the finalized sample's events that pass the thresholds, on the device (asynchronous)."""
        _check(self._L.bk_sample_indels(self.h, C.byref(_ffi.IndelParams(int(min_reads), int(min_af_ppm)))), self._L)

    def download_indels(self, cap=None):
        """(summary, rows) of sample_indels: min(cap, summary.reported) rows (cell, len, fwd, rev, ref_span, seq) -- len > 0 a deletion,
        < 0 an insertion --, all by default, sorted by (cell, kind, length, seq)."""
        dt = np.dtype([("cell", np.uint32), ("len", np.int32), ("fwd", np.uint32), ("rev", np.uint32), ("ref_span", np.uint32),
                       ("pad", np.uint32), ("seq", np.uint64)])
        summ, buf = self._download_events(self._L.bk_sample_download_indels, _ffi.IndelSummary(), cap, dt)
        rows = [(int(r["cell"]), int(r["len"]), int(r["fwd"]), int(r["rev"]), int(r["ref_span"]), int(r["seq"])) for r in buf]
        rows.sort(key=lambda r: (r[0], 1 if r[1] < 0 else 0, abs(r[1]), r[5]))
        return summ, rows

    def download_indel_span(self):
        """bk_sample_download_indel_span: the prefix-summed span array of all cells (after sample_indels)."""
        return self._download_event_span(self._L.bk_sample_download_indel_span)

    def sample_consensus_indels(self):
        """bk_sample_consensus_indels: the sample's indel events applied to its consensus letters at the last sample_consensus's
        parameters, on the device (asynchronous); after sample_consensus and sample_indels."""
        _check(self._L.bk_sample_consensus_indels(self.h), self._L)

    def download_consensus_indels(self, cap=None):
        """(summary, rows) of sample_consensus_indels: min(cap, summary.accepted) rows (cell, len, support, ref_span, seq, applied) --
        len > 0 a deletion, < 0 an insertion --, all by default, sorted by (cell, kind, length, seq)."""
        dt = np.dtype([("cell", np.uint32), ("len", np.int32), ("support", np.uint32), ("ref_span", np.uint32), ("seq", np.uint64),
                       ("applied", np.uint32), ("pad", np.uint32)])
        summ = _ffi.ConsensusIndelSummary()
        if cap is None:
            _check(self._L.bk_sample_download_consensus_indels(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many rows there are)
            cap = int(summ.accepted)
        buf = np.zeros(max(1, cap), dt)
        _check(self._L.bk_sample_download_consensus_indels(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        rows = [(int(r["cell"]), int(r["len"]), int(r["support"]), int(r["ref_span"]), int(r["seq"]), int(r["applied"])) for r in buf[:min(cap, int(summ.accepted))]]
        rows.sort(key=lambda r: (r[0], 1 if r[1] < 0 else 0, abs(r[1]), r[4]))
        return summ, rows

    def junctions_enable(self, min_len=33, max_mismatches=2, table_log2=16):
        """bk_junctions_enable: junction_scan_kernel runs behind every scan of the samples that begin from now on; min_len=None disables."""
        cfg = None if min_len is None else C.byref(_ffi.JunctionConfig(int(min_len), int(max_mismatches), int(table_log2)))
        _check(self._L.bk_junctions_enable(self.h, cfg), self._L)

    def sample_junctions(self, min_reads=5):
        """bk_sample_junctions: the finalized sample's junctions with at least min_reads reads, on the device (asynchronous)."""
        _check(self._L.bk_sample_junctions(self.h, C.byref(_ffi.JunctionParams(int(min_reads)))), self._L)

    def download_junctions(self, cap=None):
        """(summary, rows) of sample_junctions: min(cap, summary.reported) rows (cell, len, fwd, rev, span_donor, span_acceptor), all by
        default, sorted by (cell, len)."""
        summ, buf = self._download_events(self._L.bk_sample_download_junctions, _ffi.JunctionSummary(), cap, np.uint32, 6)
        return summ, sorted(tuple(int(v) for v in r) for r in buf)

    def download_junction_span(self):
        """bk_sample_download_junction_span: the prefix-summed span array of all cells (after sample_junctions)."""
        return self._download_event_span(self._L.bk_sample_download_junction_span)

    def copybacks_enable(self, max_mismatches=2, table_log2=16):
        """bk_copybacks_enable: copyback_scan_kernel runs behind every scan of the samples that begin from now on; max_mismatches=None
        disables."""
        cfg = None if max_mismatches is None else C.byref(_ffi.CopybackConfig(int(max_mismatches), int(table_log2)))
        _check(self._L.bk_copybacks_enable(self.h, cfg), self._L)

    def sample_copybacks(self, min_reads=5, min_dist=0):
        """bk_sample_copybacks: the finalized sample's copy-backs with at least min_reads reads and hi - lo >= min_dist, on the device
        (asynchronous)."""
        _check(self._L.bk_sample_copybacks(self.h, C.byref(_ffi.CopybackParams(int(min_reads), int(min_dist)))), self._L)

    def download_copybacks(self, cap=None):
        """(summary, rows) of sample_copybacks: min(cap, summary.reported) rows (lo, hi, kind, lo_first, hi_first, span_lo, span_hi, 0),
        all by default, sorted."""
        summ, buf = self._download_events(self._L.bk_sample_download_copybacks, _ffi.CopybackSummary(), cap, np.uint32, 8)
        return summ, sorted(tuple(int(v) for v in r) for r in buf)

    def download_copyback_span(self):
        """bk_sample_download_copyback_span: the prefix-summed span array of all cells (after sample_copybacks)."""
        return self._download_event_span(self._L.bk_sample_download_copyback_span)

    def chimeras_enable(self, max_mismatches=2, table_log2=16):
        """bk_chimeras_enable: chimera_scan_kernel runs behind every scan of the samples that begin from now on; max_mismatches=None
        disables."""
        cfg = None if max_mismatches is None else C.byref(_ffi.ChimeraConfig(int(max_mismatches), int(table_log2)))
        _check(self._L.bk_chimeras_enable(self.h, cfg), self._L)

    def sample_chimeras(self, min_reads=5):
        """bk_sample_chimeras: the finalized sample's junctions between two sequences with at least min_reads reads, on the device
        (asynchronous)."""
        _check(self._L.bk_sample_chimeras(self.h, C.byref(_ffi.ChimeraParams(int(min_reads)))), self._L)

    def download_chimeras(self, cap=None):
        """(summary, rows) of sample_chimeras: min(cap, summary.reported) rows (lo, hi, sides, lo_first, hi_first, span_lo, span_hi, 0),
        all by default, sorted."""
        summ, buf = self._download_events(self._L.bk_sample_download_chimeras, _ffi.ChimeraSummary(), cap, np.uint32, 8)
        return summ, sorted(tuple(int(v) for v in r) for r in buf)

    def download_chimera_span(self):
        """bk_sample_download_chimera_span: the prefix-summed span array of all cells (after sample_chimeras)."""
        return self._download_event_span(self._L.bk_sample_download_chimera_span)

    def breakends_enable(self, min_clip=20, max_mismatches=2, table_log2=16):
        """bk_breakends_enable: breakend_scan_kernel runs behind every scan of the samples that begin from now on; min_clip=None
        disables."""
        cfg = None if min_clip is None else C.byref(_ffi.BreakendConfig(int(min_clip), int(max_mismatches), int(table_log2)))
        _check(self._L.bk_breakends_enable(self.h, cfg), self._L)

    def sample_breakends(self, min_reads=5):
        """bk_sample_breakends: the finalized sample's breakends with at least min_reads reads, on the device (asynchronous)."""
        _check(self._L.bk_sample_breakends(self.h, C.byref(_ffi.BreakendParams(int(min_reads)))), self._L)

    def download_breakends(self, cap=None):
        """(summary, rows) of sample_breakends: min(cap, summary.reported) rows (cell, tag, side, fwd, rev, site_reads, span, 0), all by
        default, sorted."""
        summ, buf = self._download_events(self._L.bk_sample_download_breakends, _ffi.BreakendSummary(), cap, np.uint32, 8)
        return summ, sorted(tuple(int(v) for v in r) for r in buf)

    def download_breakend_span(self):
        """bk_sample_download_breakend_span: the prefix-summed span array of all cells (after sample_breakends)."""
        return self._download_event_span(self._L.bk_sample_download_breakend_span)

    def duplications_enable(self, min_len=33, max_mismatches=2, table_log2=16):
        """bk_duplications_enable: duplication_scan_kernel runs behind every scan of the samples that begin from now on; min_len=None disables."""
        cfg = None if min_len is None else C.byref(_ffi.DuplicationConfig(int(min_len), int(max_mismatches), int(table_log2)))
        _check(self._L.bk_duplications_enable(self.h, cfg), self._L)

    def sample_duplications(self, min_reads=5):
        """bk_sample_duplications: the finalized sample's duplications with at least min_reads reads, on the device (asynchronous)."""
        _check(self._L.bk_sample_duplications(self.h, C.byref(_ffi.DuplicationParams(int(min_reads)))), self._L)

    def download_duplications(self, cap=None):
        """(summary, rows) of sample_duplications: min(cap, summary.reported) rows (cell, len, fwd, rev, span_start, span_end), all by
        default, sorted by (cell, len)."""
        summ, buf = self._download_events(self._L.bk_sample_download_duplications, _ffi.DuplicationSummary(), cap, np.uint32, 6)
        return summ, sorted(tuple(int(v) for v in r) for r in buf)

    def download_duplication_span(self):
        """bk_sample_download_duplication_span: the prefix-summed span array of all cells (after sample_duplications)."""
        return self._download_event_span(self._L.bk_sample_download_duplication_span)

    def linkage_enable(self, max_mismatches=8, initial_rows=1 << 16):
        """bk_link_enable: link_scan_kernel runs behind every scan of the samples that begin from now on and keeps a row per placed
        record; max_mismatches=None disables."""
        cfg = None if max_mismatches is None else C.byref(_ffi.LinkConfig(int(max_mismatches), int(initial_rows)))
        _check(self._L.bk_link_enable(self.h, cfg), self._L)

    def sample_linkage(self, cells, max_dist=1000):
        """bk_sample_linkage: the 16 counters of every pair of the sites `cells` (strictly ascending) at most max_dist apart, counted
        from the finalized sample's rows on the device (asynchronous)."""
        arr = np.ascontiguousarray(np.asarray(cells, np.int64).astype(np.uint32))
        _check(self._L.bk_sample_linkage(self.h, arr.ctypes.data_as(C.c_void_p), len(arr), int(max_dist)), self._L)

    def download_linkage(self, cap=None):
        """(summary, pairs) of sample_linkage: pairs = [(site_a, site_b, [16 counters: 4 * base at a + base at b])] in (i, j) order,
        min(cap, summary.n_pairs) of them, all by default."""
        summ = _ffi.LinkSummary()
        if cap is None:
            _check(self._L.bk_sample_download_linkage(self.h, C.byref(summ), None, 0), self._L)
            cap = int(summ.n_pairs)
        buf = np.zeros((max(1, cap), 18), np.uint32)
        _check(self._L.bk_sample_download_linkage(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, [(int(r[0]), int(r[1]), [int(v) for v in r[2:]]) for r in buf[:min(cap, int(summ.n_pairs))]]

    def download_link_rows(self, cap=None, raw=False):
        """bk_sample_download_link_rows: the finalized sample's row store as [(cell0, n, strand, ((offset, base), ...))], sorted.
        raw=True: the rows as they lie in the store, an (n, 32) uint8 array of bk_link_row, not decoded and not sorted."""
        summ = _ffi.LinkSummary()
        _check(self._L.bk_sample_download_linkage(self.h, C.byref(summ), None, 0), self._L)   # (how many rows the store holds)
        cap = int(summ.placed) if cap is None else min(int(cap), int(summ.placed))
        buf = np.zeros((max(1, cap), 32), np.uint8)
        _check(self._L.bk_sample_download_link_rows(self.h, buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return buf[:cap] if raw else link_rows(buf[:cap])

    def sample_codons(self, regions):
        """bk_sample_codons: for every codon of the regions [(cell0, n_codons), ...] (forward-strand cells, any order) the rows of the
        finalized sample's store by the triplet they carry there, counted on the device (asynchronous); needs linkage_enable."""
        arr = np.ascontiguousarray(np.asarray(regions, np.int64).reshape(-1, 2).astype(np.uint32))
        _check(self._L.bk_sample_codons(self.h, arr.ctypes.data_as(C.c_void_p), len(arr)), self._L)

    def download_codons(self, cap=None):
        """(summary, counts) of sample_codons: counts[codon][16 b0 + 4 b1 + b2] as an (n, 64) uint32 array in the caller's codon
        numbering, n = min(cap, summary.n_codons), all by default."""
        summ = _ffi.CodonSummary()
        if cap is None:
            _check(self._L.bk_sample_download_codons(self.h, C.byref(summ), None, 0), self._L)
            cap = int(summ.n_codons)
        buf = np.zeros((max(1, cap), 64), np.uint32)
        _check(self._L.bk_sample_download_codons(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, buf[:min(cap, int(summ.n_codons))]

    def sample_haplotypes(self, regions, table_log2=16):
        """bk_sample_haplotypes: for every region [(cell0, len), ...] (forward-strand cells, any order) the rows of the finalized
        sample's store that span it, by the list of substitutions they carry inside it, counted on the device (asynchronous) in a
        table of 2^table_log2 slots; needs linkage_enable."""
        arr = np.ascontiguousarray(np.asarray(regions, np.int64).reshape(-1, 2).astype(np.uint32))
        _check(self._L.bk_sample_haplotypes(self.h, arr.ctypes.data_as(C.c_void_p), len(arr), int(table_log2)), self._L)

    def download_haplotypes(self, cap=None):
        """(summary, cover, ref_count, entries) of sample_haplotypes: cover and ref_count as uint32 arrays in the regions' order,
        entries [(region, count, ((offset, base), ...))] in the defined order, min(cap, summary.entries) of them, all by default.
        A table that dropped counts raises BronkoError (status -6) with .hap = (summary, cover, ref_count): those stay exact."""
        summ = _ffi.HapSummary()
        rc = self._L.bk_sample_download_haplotypes(self.h, C.byref(summ), None, None, None, 0)   # (sizes; -6 still fills the summary)
        if rc != -6:
            _check(rc, self._L)
        n = int(summ.n_regions)
        cover, ref = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32)
        cap = int(summ.entries) if cap is None else int(cap)
        buf = np.zeros((max(1, cap), 40), np.uint8)
        rc = self._L.bk_sample_download_haplotypes(self.h, C.byref(summ), cover.ctypes.data_as(C.c_void_p), ref.ctypes.data_as(C.c_void_p),
                                                   buf.ctypes.data_as(C.c_void_p), cap)
        if rc != 0:
            try:
                _check(rc, self._L)
            except BronkoError as err:
                err.hap = (summ, cover[:n], ref[:n])
                raise
        return summ, cover[:n], ref[:n], hap_entries(buf[:min(cap, int(summ.entries))])

    def sample_read_pileup(self, end_dist=10):
        """bk_sample_read_pileup: per cell the rows of the finalized sample's store that cover it, by the base they carry there, by
        strand and near their ends (within end_dist positions of one), counted on the device (asynchronous); needs linkage_enable."""
        _check(self._L.bk_sample_read_pileup(self.h, int(end_dist)), self._L)

    def download_read_pileup(self, cap=None):
        """(summary, cells) of sample_read_pileup: cells as an (n, 12) uint32 array -- fwd[ACGT], rev[ACGT], near[ACGT] per cell --,
        n = min(cap, summary.n_cells), all by default."""
        summ = _ffi.ReadPileupSummary()
        if cap is None:
            _check(self._L.bk_sample_download_read_pileup(self.h, C.byref(summ), None, 0), self._L)
            cap = int(summ.n_cells)
        buf = np.zeros((max(1, cap), 12), np.uint32)
        _check(self._L.bk_sample_download_read_pileup(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, buf[:min(cap, int(summ.n_cells))]

    def cohort_set(self, letters):
        """bk_cohort_set: the consensus letters of a cohort, an (n_samples, positions) uint8 array, uploaded and packed into bit
        planes on the device; replaces an earlier cohort.  Between samples only."""
        a = np.ascontiguousarray(letters, np.uint8)
        if a.ndim != 2:
            raise ValueError("cohort_set takes a 2-d array: a row of letters per sample")
        _check(self._L.bk_cohort_set(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1]), self._L)
        self._cohort_n = int(a.shape[0])

    def cohort_distances(self, row0=0, n_rows=None):
        """bk_cohort_distances: (diff, compared) of the rows [row0, row0 + n_rows) against every sample of the cohort, two
        (n_rows, n_samples) uint32 arrays; all rows from row0 on by default."""
        n = int(getattr(self, "_cohort_n", 0))
        if n_rows is None:
            n_rows = max(0, n - int(row0))
        diff = np.zeros((max(1, int(n_rows)), max(1, n)), np.uint32)
        compared = np.zeros_like(diff)
        _check(self._L.bk_cohort_distances(self.h, int(row0), int(n_rows), diff.ctypes.data_as(C.c_void_p), compared.ctypes.data_as(C.c_void_p)), self._L)
        return diff[:int(n_rows), :n], compared[:int(n_rows), :n]

    def cohort_mst(self, min_compared=0, nearest=True, rounds=True):
        """bk_cohort_mst: the minimum spanning forest of the cohort under the edge order (diff, lo, hi) over the pairs that compared
        at least max(1, min_compared) positions: (edges, nearest, rounds) -- edges an (E, 4) uint32 array of lo, hi, diff, compared,
        ascending in the edge order; nearest an (n, 3) uint32 array of sample (0xffffffff: none), diff, compared; rounds the Boruvka
        rounds that added an edge.  nearest=False / rounds=False pass NULL and return None there."""
        n = int(getattr(self, "_cohort_n", 0))
        cap = max(1, n)
        edges = np.zeros((cap, 4), np.uint32)
        near = np.zeros((cap, 3), np.uint32) if nearest else None
        n_edges = C.c_uint64(0)
        n_rounds = C.c_uint32(0)
        _check(self._L.bk_cohort_mst(self.h, int(min_compared), edges.ctypes.data_as(C.POINTER(_ffi.MstEdge)), cap, C.byref(n_edges),
                                     near.ctypes.data_as(C.POINTER(_ffi.MstNearest)) if nearest else None,
                                     C.byref(n_rounds) if rounds else None), self._L)
        return edges[:int(n_edges.value)], (near[:n] if nearest else None), (int(n_rounds.value) if rounds else None)

    def cohort_set_minor(self, masks):
        """bk_cohort_set_minor: the present masks of the cohort's samples, an (n_samples, positions) uint8 array shaped like the
        letters of cohort_set, uploaded and packed into four minor planes per sample; a later cohort_set drops them."""
        a = np.ascontiguousarray(masks, np.uint8)
        if a.ndim != 2:
            raise ValueError("cohort_set_minor takes a 2-d array: a row of masks per sample")
        _check(self._L.bk_cohort_set_minor(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1]), self._L)

    def cohort_explained(self, row0=0, n_rows=None):
        """bk_cohort_explained: (explained, minor_sites) of the rows [row0, row0 + n_rows) -- the recipients -- against every sample of
        the cohort, an (n_rows, n_samples) and an (n_rows,) uint32 array; all rows from row0 on by default."""
        n = int(getattr(self, "_cohort_n", 0))
        if n_rows is None:
            n_rows = max(0, n - int(row0))
        explained = np.zeros((max(1, int(n_rows)), max(1, n)), np.uint32)
        sites = np.zeros(max(1, int(n_rows)), np.uint32)
        _check(self._L.bk_cohort_explained(self.h, int(row0), int(n_rows), explained.ctypes.data_as(C.c_void_p), sites.ctypes.data_as(C.c_void_p)), self._L)
        return explained[:int(n_rows), :n], sites[:int(n_rows)]

    def cohort_clear(self):
        """bk_cohort_clear: frees the cohort's device memory (fine without a cohort)."""
        _check(self._L.bk_cohort_clear(self.h), self._L)
        self._cohort_n = 0

    def regions_set(self, regions):
        """bk_regions_set: the regions [(file_id, seq, start, end), ...] whose depths sample_region_depths reports; [] clears them."""
        arr = (_ffi.Region * max(1, len(regions)))(*[_ffi.Region(*(int(v) for v in r[:4])) for r in regions])
        _check(self._L.bk_regions_set(self.h, arr, len(regions)), self._L)

    def sample_region_depths(self, min_depth=10):
        """The depth numbers of every region of the genome sample_call selected, on the device (asynchronous)."""
        _check(self._L.bk_sample_region_depths(self.h, int(min_depth)), self._L)

    def download_region_depths(self, cap=None):
        """(summary, rows) of sample_region_depths: min(cap, summary.n_regions) rows (sum, min, max, median, covered), all by default."""
        summ = _ffi.RegionSummary()
        if cap is None:
            _check(self._L.bk_sample_download_region_depths(self.h, C.byref(summ), None, 0), self._L)   # (the summary first: how many rows there are)
            cap = int(summ.n_regions)
        buf = np.zeros((max(1, cap), 5), np.uint64)
        _check(self._L.bk_sample_download_region_depths(self.h, C.byref(summ), buf.ctypes.data_as(C.c_void_p), cap), self._L)
        return summ, [tuple(int(v) for v in r) for r in buf[:min(cap, int(summ.n_regions))]]

    def timing_enable(self, on=True):
        _check(self._L.bk_timing_enable(self.h, int(on)), self._L)

    def timing_read(self, reset=True):
        ms = (C.c_double * 4)()
        n = (C.c_uint64 * 4)()
        _check(self._L.bk_timing_read(self.h, ms, n, int(reset)), self._L)
        return list(ms), list(n)


def hap_entries(raw):
    """[n][40] bytes of bk_hap_entry as [(region, count, ((offset, base), ...))], in the order given.  An entry that the device cannot
    have written (no or more than 8 substitutions, a pad byte or an entry behind n_mm that is not zero) raises ValueError."""
    out = []
    for i, r in enumerate(np.asarray(raw, np.uint8).reshape(-1, 40)):
        b = r.tobytes()
        n_mm = b[8]
        if n_mm < 1 or n_mm > 8 or any(b[9:16]) or any(b[16 + 3 * n_mm:]):
            raise ValueError("entry %d of the haplotype list is no haplotype: %s" % (i, b.hex()))
        mm = tuple((b[16 + 3 * t] | (b[17 + 3 * t] << 8), b[18 + 3 * t]) for t in range(n_mm))
        out.append((int.from_bytes(b[:4], "little"), int.from_bytes(b[4:8], "little"), mm))
    return out


def link_rows(raw):
    """[n][32] bytes of bk_link_row as [(cell0, n, strand, ((offset, base), ...))], sorted.  A row that no placed record can have
    left (n = 0, more than 8 mismatches, an entry behind n_mm that is not zero) raises ValueError."""
    out = []
    for i, r in enumerate(np.asarray(raw, np.uint8).reshape(-1, 32)):
        b = r.tobytes()
        n, n_mm = b[4] | (b[5] << 8), b[7]
        if n == 0 or n_mm > 8 or any(b[8 + 3 * n_mm:]):
            raise ValueError("row %d of the row store is no placed record's: %s" % (i, b.hex()))
        mm = tuple((b[8 + 3 * t] | (b[9 + 3 * t] << 8), b[10 + 3 * t]) for t in range(n_mm))
        out.append((int.from_bytes(b[:4], "little"), n, b[6], mm))
    out.sort()
    return out
