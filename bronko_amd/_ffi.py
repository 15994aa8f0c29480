"""ctypes binding of include/bronko_hip.h (libbronko_hip.so).  No fallbacks: a missing library is an error."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (BRONKO_HIP_LIB: another build of the same library, for A/B timing of two builds in one run -- tools/ab.sh; the harness reads it, the
# library itself reads no environment)
LIB_PATH = os.environ.get("BRONKO_HIP_LIB") or os.path.join(_HERE, "libbronko_hip.so")
# the -DBK_TESTING build of the same sources: BK_* environment variables that force a code path exist only there
TESTING_LIB_PATH = os.environ.get("BRONKO_HIP_TESTING_LIB") or os.path.join(_HERE, "libbronko_hip_testing.so")


class BucketInfo(C.Structure):  # include/bronko_hip.h bk_bucket_info == build.rs:52-60
    _fields_ = [("file_id", C.c_uint16), ("seq_id", C.c_uint8), ("location", C.c_uint32),
                ("idx", C.c_uint8), ("canonical", C.c_uint8)]


class IndexDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("n_buckets", C.c_uint64), ("bucket_ids", C.c_void_p), ("bucket_off", C.c_void_p),
                ("entries", C.c_void_p), ("n_entries", C.c_uint64), ("n_files", C.c_int32), ("n_seqs", C.c_void_p),
                ("seq_lens", C.c_void_p), ("seqs", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [("n_fixed", C.c_int32), ("use_full_kmer", C.c_int32), ("ci", C.c_uint64), ("cs", C.c_uint64),
                ("cx", C.c_uint64), ("device", C.c_int32), ("full_kmer_stats", C.c_int32),
                ("kmer_table_log2", C.c_uint32), ("pileup_selected_only", C.c_uint32)]


class CallParams(C.Structure):  # include/bronko_hip.h bk_call_params
    _fields_ = [("k", C.c_int32), ("no_end_filter", C.c_int32), ("no_strand_filter", C.c_int32), ("no_strand_balance_filter", C.c_int32),
                ("min_af", C.c_double), ("strand_balance_ratio", C.c_double), ("strand_odds_max", C.c_double),
                ("variant_multiplier", C.c_double), ("n_per_strand", C.c_uint64), ("min_depth", C.c_uint64),
                ("min_variant_depth", C.c_uint64)]


class CallRecord(C.Structure):  # bk_call_record
    _fields_ = [("seq_id", C.c_int32), ("ref_base", C.c_uint8), ("alt_base", C.c_uint8), ("pad", C.c_uint16), ("pos", C.c_uint64),
                ("fwd_ref", C.c_uint64), ("rev_ref", C.c_uint64), ("fwd_alt", C.c_uint64), ("rev_alt", C.c_uint64),
                ("depth", C.c_uint64), ("af", C.c_double), ("sor", C.c_double)]


class CallSummary(C.Structure):  # bk_call_summary
    _fields_ = [("file_id", C.c_int32), ("pad", C.c_uint32), ("n_records", C.c_uint64), ("n_major", C.c_uint64), ("n_minor", C.c_uint64),
                ("covered", C.c_uint64), ("positions", C.c_uint64), ("coverage", C.c_uint64)]


class ConsensusParams(C.Structure):  # bk_consensus_params
    _fields_ = [("min_depth", C.c_uint64), ("min_freq", C.c_double)]


class ConsensusSummary(C.Structure):  # bk_consensus_summary
    _fields_ = [("file_id", C.c_int32), ("pad", C.c_uint32), ("positions", C.c_uint64), ("called", C.c_uint64), ("ambiguous", C.c_uint64),
                ("masked", C.c_uint64), ("substitutions", C.c_uint64)]


class MinorParams(C.Structure):  # bk_minor_params
    _fields_ = [("min_reads", C.c_uint64), ("min_freq", C.c_double)]


class MinorSummary(C.Structure):  # bk_minor_summary
    _fields_ = [("file_id", C.c_int32), ("pad", C.c_uint32), ("positions", C.c_uint64), ("mixed", C.c_uint64), ("present", C.c_uint64)]


class Region(C.Structure):  # bk_region
    _fields_ = [("file_id", C.c_int32), ("seq", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32)]


class RegionDepth(C.Structure):  # bk_region_depth
    _fields_ = [("sum", C.c_uint64), ("min", C.c_uint64), ("max", C.c_uint64), ("median", C.c_uint64), ("covered", C.c_uint64)]


class IndelConfig(C.Structure):  # bk_indel_config
    _fields_ = [("max_len", C.c_uint32), ("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class IndelParams(C.Structure):  # bk_indel_params
    _fields_ = [("min_reads", C.c_uint64), ("min_af_ppm", C.c_uint32)]


class IndelSummary(C.Structure):  # bk_indel_summary
    _fields_ = [("records", C.c_uint64), ("anchored", C.c_uint64), ("ref_spanning", C.c_uint64), ("supporting", C.c_uint64),
                ("discordant", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64), ("overflow", C.c_int32)]


class ConsensusIndelSummary(C.Structure):  # bk_consensus_indel_summary
    _fields_ = [("candidates", C.c_uint64), ("accepted", C.c_uint64), ("applied", C.c_uint64), ("contested", C.c_uint64), ("deletions", C.c_uint64),
                ("insertions", C.c_uint64), ("deleted_bases", C.c_uint64), ("inserted_bases", C.c_uint64), ("frameshifts", C.c_uint64),
                ("file_id", C.c_int32), ("overflow", C.c_int32)]


class JunctionConfig(C.Structure):  # bk_junction_config
    _fields_ = [("min_len", C.c_uint32), ("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class JunctionParams(C.Structure):  # bk_junction_params
    _fields_ = [("min_reads", C.c_uint64)]


class JunctionSummary(C.Structure):  # bk_junction_summary
    _fields_ = [("records", C.c_uint64), ("anchored", C.c_uint64), ("ref_spanning", C.c_uint64), ("supporting", C.c_uint64), ("short_", C.c_uint64),
                ("backward", C.c_uint64), ("discordant", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64), ("overflow", C.c_int32)]


class CopybackConfig(C.Structure):  # bk_copyback_config
    _fields_ = [("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class CopybackParams(C.Structure):  # bk_copyback_params
    _fields_ = [("min_reads", C.c_uint64), ("min_dist", C.c_uint32)]


class CopybackSummary(C.Structure):  # bk_copyback_summary
    _fields_ = [("records", C.c_uint64), ("same_strand", C.c_uint64), ("ref_spanning", C.c_uint64), ("switched", C.c_uint64), ("supporting", C.c_uint64),
                ("discordant", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64), ("overflow", C.c_int32)]


class ChimeraConfig(C.Structure):  # bk_chimera_config
    _fields_ = [("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class ChimeraParams(C.Structure):  # bk_chimera_params
    _fields_ = [("min_reads", C.c_uint64)]


class ChimeraSummary(C.Structure):  # bk_chimera_summary
    _fields_ = [("records", C.c_uint64), ("same_strand", C.c_uint64), ("ref_spanning", C.c_uint64), ("crossed", C.c_uint64), ("supporting", C.c_uint64),
                ("discordant", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64), ("overflow", C.c_int32)]


class BreakendConfig(C.Structure):  # bk_breakend_config
    _fields_ = [("min_clip", C.c_uint32), ("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class BreakendParams(C.Structure):  # bk_breakend_params
    _fields_ = [("min_reads", C.c_uint64)]


class BreakendSummary(C.Structure):  # bk_breakend_summary
    _fields_ = [("records", C.c_uint64), ("one_anchor", C.c_uint64), ("ref_spanning", C.c_uint64), ("supporting", C.c_uint64), ("short_", C.c_uint64),
                ("through", C.c_uint64), ("discordant", C.c_uint64), ("unplaced", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64),
                ("overflow", C.c_int32)]


class DuplicationConfig(C.Structure):  # bk_duplication_config
    _fields_ = [("min_len", C.c_uint32), ("max_mismatches", C.c_uint32), ("table_log2", C.c_uint32)]


class DuplicationParams(C.Structure):  # bk_duplication_params
    _fields_ = [("min_reads", C.c_uint64)]


class DuplicationSummary(C.Structure):  # bk_duplication_summary
    _fields_ = [("records", C.c_uint64), ("anchored", C.c_uint64), ("ref_spanning", C.c_uint64), ("supporting", C.c_uint64), ("short_", C.c_uint64),
                ("forward", C.c_uint64), ("discordant", C.c_uint64), ("candidates", C.c_uint64), ("reported", C.c_uint64), ("overflow", C.c_int32)]


class CodonSummary(C.Structure):  # bk_codon_summary
    _fields_ = [("rows", C.c_uint64), ("n_codons", C.c_uint64), ("n_regions", C.c_uint32)]


class HapSummary(C.Structure):  # bk_hap_summary
    _fields_ = [("rows", C.c_uint64), ("entries", C.c_uint64), ("dropped", C.c_uint64), ("n_regions", C.c_uint32), ("table_log2", C.c_uint32)]


class ReadPileupCell(C.Structure):  # bk_read_pileup_cell
    _fields_ = [("fwd", C.c_uint32 * 4), ("rev", C.c_uint32 * 4), ("near", C.c_uint32 * 4)]


class ReadPileupSummary(C.Structure):  # bk_read_pileup_summary
    _fields_ = [("rows", C.c_uint64), ("n_cells", C.c_uint64), ("end_dist", C.c_uint32), ("pad", C.c_uint32), ("covered", C.c_uint64), ("bases", C.c_uint64)]


class LinkConfig(C.Structure):  # bk_link_config
    _fields_ = [("max_mismatches", C.c_uint32), ("initial_rows", C.c_uint64)]


class LinkSummary(C.Structure):  # bk_link_summary
    _fields_ = [("records", C.c_uint64), ("placed", C.c_uint64), ("unplaced", C.c_uint64), ("discordant", C.c_uint64), ("n_pairs", C.c_uint64),
                ("n_sites", C.c_uint32), ("max_dist", C.c_uint32)]


class RegionSummary(C.Structure):  # bk_region_summary
    _fields_ = [("file_id", C.c_int32), ("n_regions", C.c_uint32), ("full", C.c_uint64), ("partial", C.c_uint64), ("empty", C.c_uint64)]


class MstEdge(C.Structure):  # bk_mst_edge
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32), ("diff", C.c_uint32), ("compared", C.c_uint32)]


class MstNearest(C.Structure):  # bk_mst_nearest
    _fields_ = [("sample", C.c_uint32), ("diff", C.c_uint32), ("compared", C.c_uint32)]


class BuiltIndex(C.Structure):  # bk_built_index
    _fields_ = [("n_buckets", C.c_uint64), ("n_entries", C.c_uint64), ("bucket_ids", C.c_void_p), ("bucket_off", C.c_void_p),
                ("entries", C.c_void_p)]


# every symbol include/bronko_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = ["bk_abi_version", "bk_device_count", "bk_device_memory", "bk_last_error", "bk_params_default", "bk_engine_create", "bk_engine_destroy", "bk_engine_fork", "bk_engine_fork_params", "bk_engine_get_stream",
           "bk_engine_set_stream", "bk_total_cells", "bk_n_files", "bk_n_slots", "bk_counter_len", "bk_can_shard", "bk_sample_begin",
           "bk_push_reads_packed", "bk_push_reads_packed_device", "bk_push_reads_ascii", "bk_push_reads_ascii_device", "bk_push_reads_ascii_qual", "bk_push_reads_ascii_qual_device", "bk_counters_device_ptr", "bk_sample_finalize",
           "bk_sample_finalize_shard", "bk_shard_measure", "bk_shard_transport", "bk_shard_received", "bk_transport_overflow", "bk_shard_sums_device_ptr", "bk_sample_merge_shards", "bk_kmer_table_partition", "bk_kmer_table_replace",
           "bk_kmer_dump_enable", "bk_kmer_dump_size", "bk_kmer_dump_download",
           "bk_primers_set", "bk_push_reads_packed_ends", "bk_push_reads_packed_ends_device", "bk_primer_stats", "bk_pack_reads_flat_ends",
           "bk_adapters_set", "bk_adapter_stats",
           "bk_pileup_device_ptr", "bk_sample_download", "bk_sample_finish", "bk_pack_reads", "bk_pack_reads_flat",
           "bk_timing_enable", "bk_timing_read", "bk_call_params_default", "bk_sample_call", "bk_sample_download_calls", "bk_sample_download_noise",
           "bk_consensus_params_default", "bk_sample_consensus", "bk_sample_download_consensus",
           "bk_minor_params_default", "bk_sample_minor_alleles", "bk_sample_download_minor_alleles",
           "bk_regions_set", "bk_sample_region_depths", "bk_sample_download_region_depths",
           "bk_indels_enable", "bk_sample_indels", "bk_sample_download_indels", "bk_sample_download_indel_span",
           "bk_sample_consensus_indels", "bk_sample_download_consensus_indels",
           "bk_junctions_enable", "bk_sample_junctions", "bk_sample_download_junctions", "bk_sample_download_junction_span",
           "bk_copybacks_enable", "bk_sample_copybacks", "bk_sample_download_copybacks", "bk_sample_download_copyback_span",
           "bk_chimeras_enable", "bk_sample_chimeras", "bk_sample_download_chimeras", "bk_sample_download_chimera_span",
           "bk_breakends_enable", "bk_sample_breakends", "bk_sample_download_breakends", "bk_sample_download_breakend_span",
           "bk_duplications_enable", "bk_sample_duplications", "bk_sample_download_duplications", "bk_sample_download_duplication_span",
           "bk_link_enable", "bk_sample_linkage", "bk_sample_download_linkage", "bk_sample_download_link_rows",
           "bk_sample_codons", "bk_sample_download_codons", "bk_sample_haplotypes", "bk_sample_download_haplotypes",
           "bk_sample_read_pileup", "bk_sample_download_read_pileup",
           "bk_cohort_set", "bk_cohort_distances", "bk_cohort_clear", "bk_cohort_mst", "bk_cohort_set_minor", "bk_cohort_explained",
           "bk_build_index", "bk_built_index_free", "bk_build_last_error"]

_libs = {}
_testing = False


def use_testing_library(flag=True):
    """Engines created from now on bind libbronko_hip_testing.so (tests that force a path through a BK_* variable, profiling
    tools); the product and bench.py never call this."""
    global _testing
    _testing = bool(flag)


def load(testing=None):
    testing = _testing if testing is None else bool(testing)
    if testing in _libs:
        return _libs[testing]
    path = TESTING_LIB_PATH if testing else LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError("bronko_amd: %s is missing -- build it with `make -C bronko_amd/csrc` "
                           "(or python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % path)
    L = C.CDLL(path)
    vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32
    L.bk_abi_version.restype = C.c_int
    L.bk_device_count.restype = C.c_int
    L.bk_device_memory.restype = C.c_int
    L.bk_device_memory.argtypes = [C.c_int, C.POINTER(u64), C.POINTER(u64)]
    L.bk_last_error.restype = C.c_char_p
    L.bk_params_default.argtypes = [C.POINTER(Params)]
    L.bk_engine_create.restype = C.c_int
    L.bk_engine_create.argtypes = [C.POINTER(IndexDesc), C.POINTER(Params), C.POINTER(vp)]
    L.bk_engine_destroy.argtypes = [vp]
    L.bk_engine_get_stream.restype = vp
    L.bk_engine_get_stream.argtypes = [vp]
    L.bk_engine_fork.restype = C.c_int
    L.bk_engine_fork.argtypes = [vp, C.POINTER(vp)]
    L.bk_engine_fork_params.restype = C.c_int
    L.bk_engine_fork_params.argtypes = [vp, C.POINTER(Params), C.POINTER(vp)]
    L.bk_push_reads_ascii_device.restype = C.c_int
    L.bk_push_reads_ascii_device.argtypes = [vp, C.c_int, vp, vp, u64, u64, u32]
    L.bk_engine_set_stream.restype = C.c_int
    L.bk_engine_set_stream.argtypes = [vp, vp]
    for n, rt in (("bk_total_cells", u64), ("bk_n_files", i32), ("bk_n_slots", u64), ("bk_counter_len", u64)):
        getattr(L, n).restype = rt
        getattr(L, n).argtypes = [vp]
    L.bk_sample_begin.restype = C.c_int
    L.bk_sample_begin.argtypes = [vp]
    L.bk_push_reads_packed.restype = C.c_int
    L.bk_push_reads_packed.argtypes = [vp, C.c_int, vp, u32, vp, u64]
    L.bk_push_reads_packed_device.restype = C.c_int
    L.bk_push_reads_packed_device.argtypes = [vp, C.c_int, vp, u32, vp, u64]
    L.bk_push_reads_ascii.restype = C.c_int
    L.bk_push_reads_ascii.argtypes = [vp, C.c_int, vp, vp, u64]
    L.bk_push_reads_ascii_qual.restype = C.c_int
    L.bk_push_reads_ascii_qual.argtypes = [vp, C.c_int, vp, vp, vp, u64, C.c_int]
    L.bk_push_reads_ascii_qual_device.restype = C.c_int
    L.bk_push_reads_ascii_qual_device.argtypes = [vp, C.c_int, vp, vp, vp, u64, u64, u32, C.c_int]
    L.bk_counters_device_ptr.restype = C.c_int
    L.bk_counters_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.bk_sample_finalize.restype = C.c_int
    L.bk_sample_finalize.argtypes = [vp, C.c_int]
    L.bk_sample_finalize_shard.restype = C.c_int
    L.bk_sample_finalize_shard.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.bk_shard_measure.restype = C.c_int
    L.bk_shard_measure.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.bk_shard_transport.restype = C.c_int
    L.bk_shard_transport.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp)]
    L.bk_shard_received.restype = C.c_int
    L.bk_shard_received.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.bk_transport_overflow.restype = C.c_int
    L.bk_transport_overflow.argtypes = [vp, C.POINTER(C.c_int)]
    L.bk_kmer_table_partition.restype = C.c_int
    L.bk_kmer_table_partition.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.bk_kmer_table_replace.restype = C.c_int
    L.bk_kmer_table_replace.argtypes = [vp, vp, vp, u64]
    L.bk_kmer_dump_enable.restype = C.c_int
    L.bk_kmer_dump_enable.argtypes = [vp, u32]
    L.bk_kmer_dump_size.restype = C.c_int
    L.bk_kmer_dump_size.argtypes = [vp, C.c_int, C.POINTER(u64), C.POINTER(u64)]
    L.bk_kmer_dump_download.restype = C.c_int
    L.bk_kmer_dump_download.argtypes = [vp, C.c_int, vp, vp, u64]
    L.bk_shard_sums_device_ptr.restype = C.c_int
    L.bk_shard_sums_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.bk_sample_merge_shards.restype = C.c_int
    L.bk_sample_merge_shards.argtypes = [vp]
    L.bk_pileup_device_ptr.restype = C.c_int
    L.bk_pileup_device_ptr.argtypes = [vp, C.POINTER(vp)]
    L.bk_sample_download.restype = C.c_int
    L.bk_sample_download.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bk_sample_finish.restype = C.c_int
    L.bk_sample_finish.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bk_pack_reads.restype = u64
    L.bk_pack_reads.argtypes = [vp, vp, u64, i32, u32, vp, vp, u64]
    L.bk_pack_reads_flat.restype = u64
    L.bk_pack_reads_flat.argtypes = [vp, vp, u64, i32, u32, vp, vp, u64]
    L.bk_pack_reads_flat_ends.restype = u64
    L.bk_pack_reads_flat_ends.argtypes = [vp, vp, u64, i32, u32, vp, vp, vp, u64]
    L.bk_primers_set.restype = C.c_int
    L.bk_primers_set.argtypes = [vp, vp, vp, u32, C.c_int]
    L.bk_push_reads_packed_ends.restype = C.c_int
    L.bk_push_reads_packed_ends.argtypes = [vp, C.c_int, vp, u32, vp, vp, u64]
    L.bk_push_reads_packed_ends_device.restype = C.c_int
    L.bk_push_reads_packed_ends_device.argtypes = [vp, C.c_int, vp, u32, vp, vp, u64]
    L.bk_primer_stats.restype = C.c_int
    L.bk_primer_stats.argtypes = [vp, C.c_int, vp]
    L.bk_adapters_set.restype = C.c_int
    L.bk_adapters_set.argtypes = [vp, vp, vp, u32, u32, C.c_double]
    L.bk_adapter_stats.restype = C.c_int
    L.bk_adapter_stats.argtypes = [vp, C.c_int, vp]
    L.bk_call_params_default.argtypes = [C.POINTER(CallParams)]
    L.bk_sample_call.restype = C.c_int
    L.bk_sample_call.argtypes = [vp, C.c_int, C.POINTER(CallParams)]
    L.bk_sample_download_calls.restype = C.c_int
    L.bk_sample_download_calls.argtypes = [vp, C.POINTER(CallSummary), vp, u64]
    L.bk_sample_download_noise.restype = C.c_int
    L.bk_sample_download_noise.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.bk_consensus_params_default.argtypes = [C.POINTER(ConsensusParams)]
    L.bk_sample_consensus.restype = C.c_int
    L.bk_sample_consensus.argtypes = [vp, C.POINTER(ConsensusParams)]
    L.bk_sample_download_consensus.restype = C.c_int
    L.bk_sample_download_consensus.argtypes = [vp, C.POINTER(ConsensusSummary), vp, u64]
    L.bk_regions_set.restype = C.c_int
    L.bk_regions_set.argtypes = [vp, C.POINTER(Region), u64]
    L.bk_sample_region_depths.restype = C.c_int
    L.bk_sample_region_depths.argtypes = [vp, u64]
    L.bk_sample_download_region_depths.restype = C.c_int
    L.bk_sample_download_region_depths.argtypes = [vp, C.POINTER(RegionSummary), vp, u64]
    L.bk_indels_enable.restype = C.c_int
    L.bk_indels_enable.argtypes = [vp, C.POINTER(IndelConfig)]
    L.bk_sample_indels.restype = C.c_int
    L.bk_sample_indels.argtypes = [vp, C.POINTER(IndelParams)]
    L.bk_sample_download_indels.restype = C.c_int
    L.bk_sample_download_indels.argtypes = [vp, C.POINTER(IndelSummary), vp, u64]
    L.bk_sample_download_indel_span.restype = C.c_int
    L.bk_sample_download_indel_span.argtypes = [vp, vp, u64]
    L.bk_minor_params_default.argtypes = [C.POINTER(MinorParams)]
    L.bk_sample_minor_alleles.restype = C.c_int
    L.bk_sample_minor_alleles.argtypes = [vp, C.POINTER(MinorParams)]
    L.bk_sample_download_minor_alleles.restype = C.c_int
    L.bk_sample_download_minor_alleles.argtypes = [vp, C.POINTER(MinorSummary), vp, u64]
    L.bk_sample_consensus_indels.restype = C.c_int
    L.bk_sample_consensus_indels.argtypes = [vp]
    L.bk_sample_download_consensus_indels.restype = C.c_int
    L.bk_sample_download_consensus_indels.argtypes = [vp, C.POINTER(ConsensusIndelSummary), vp, u64]
    L.bk_junctions_enable.restype = C.c_int
    L.bk_junctions_enable.argtypes = [vp, C.POINTER(JunctionConfig)]
    L.bk_sample_junctions.restype = C.c_int
    L.bk_sample_junctions.argtypes = [vp, C.POINTER(JunctionParams)]
    L.bk_sample_download_junctions.restype = C.c_int
    L.bk_sample_download_junctions.argtypes = [vp, C.POINTER(JunctionSummary), vp, u64]
    L.bk_sample_download_junction_span.restype = C.c_int
    L.bk_sample_download_junction_span.argtypes = [vp, vp, u64]
    L.bk_copybacks_enable.restype = C.c_int
    L.bk_copybacks_enable.argtypes = [vp, C.POINTER(CopybackConfig)]
    L.bk_sample_copybacks.restype = C.c_int
    L.bk_sample_copybacks.argtypes = [vp, C.POINTER(CopybackParams)]
    L.bk_sample_download_copybacks.restype = C.c_int
    L.bk_sample_download_copybacks.argtypes = [vp, C.POINTER(CopybackSummary), vp, u64]
    L.bk_sample_download_copyback_span.restype = C.c_int
    L.bk_sample_download_copyback_span.argtypes = [vp, vp, u64]
    L.bk_chimeras_enable.restype = C.c_int
    L.bk_chimeras_enable.argtypes = [vp, C.POINTER(ChimeraConfig)]
    L.bk_sample_chimeras.restype = C.c_int
    L.bk_sample_chimeras.argtypes = [vp, C.POINTER(ChimeraParams)]
    L.bk_sample_download_chimeras.restype = C.c_int
    L.bk_sample_download_chimeras.argtypes = [vp, C.POINTER(ChimeraSummary), vp, u64]
    L.bk_sample_download_chimera_span.restype = C.c_int
    L.bk_sample_download_chimera_span.argtypes = [vp, vp, u64]
    L.bk_breakends_enable.restype = C.c_int
    L.bk_breakends_enable.argtypes = [vp, C.POINTER(BreakendConfig)]
    L.bk_sample_breakends.restype = C.c_int
    L.bk_sample_breakends.argtypes = [vp, C.POINTER(BreakendParams)]
    L.bk_sample_download_breakends.restype = C.c_int
    L.bk_sample_download_breakends.argtypes = [vp, C.POINTER(BreakendSummary), vp, u64]
    L.bk_sample_download_breakend_span.restype = C.c_int
    L.bk_sample_download_breakend_span.argtypes = [vp, vp, u64]
    L.bk_duplications_enable.restype = C.c_int
    L.bk_duplications_enable.argtypes = [vp, C.POINTER(DuplicationConfig)]
    L.bk_sample_duplications.restype = C.c_int
    L.bk_sample_duplications.argtypes = [vp, C.POINTER(DuplicationParams)]
    L.bk_sample_download_duplications.restype = C.c_int
    L.bk_sample_download_duplications.argtypes = [vp, C.POINTER(DuplicationSummary), vp, u64]
    L.bk_sample_download_duplication_span.restype = C.c_int
    L.bk_sample_download_duplication_span.argtypes = [vp, vp, u64]
    L.bk_link_enable.restype = C.c_int
    L.bk_link_enable.argtypes = [vp, C.POINTER(LinkConfig)]
    L.bk_sample_linkage.restype = C.c_int
    L.bk_sample_linkage.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.bk_sample_download_linkage.restype = C.c_int
    L.bk_sample_download_linkage.argtypes = [vp, C.POINTER(LinkSummary), vp, u64]
    L.bk_sample_download_link_rows.restype = C.c_int
    L.bk_sample_download_link_rows.argtypes = [vp, vp, u64]
    L.bk_sample_codons.restype = C.c_int
    L.bk_sample_codons.argtypes = [vp, vp, C.c_uint32]
    L.bk_sample_download_codons.restype = C.c_int
    L.bk_sample_download_codons.argtypes = [vp, C.POINTER(CodonSummary), vp, u64]
    L.bk_sample_haplotypes.restype = C.c_int
    L.bk_sample_haplotypes.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.bk_sample_download_haplotypes.restype = C.c_int
    L.bk_sample_download_haplotypes.argtypes = [vp, C.POINTER(HapSummary), vp, vp, vp, u64]
    L.bk_sample_read_pileup.restype = C.c_int
    L.bk_sample_read_pileup.argtypes = [vp, C.c_uint32]
    L.bk_sample_download_read_pileup.restype = C.c_int
    L.bk_sample_download_read_pileup.argtypes = [vp, C.POINTER(ReadPileupSummary), vp, u64]
    L.bk_cohort_set.restype = C.c_int
    L.bk_cohort_set.argtypes = [vp, vp, u64, u64]
    L.bk_cohort_distances.restype = C.c_int
    L.bk_cohort_distances.argtypes = [vp, u64, u64, vp, vp]
    L.bk_cohort_clear.restype = C.c_int
    L.bk_cohort_clear.argtypes = [vp]
    L.bk_cohort_set_minor.restype = C.c_int
    L.bk_cohort_set_minor.argtypes = [vp, vp, u64, u64]
    L.bk_cohort_explained.restype = C.c_int
    L.bk_cohort_explained.argtypes = [vp, u64, u64, vp, vp]
    L.bk_cohort_mst.restype = C.c_int
    L.bk_cohort_mst.argtypes = [vp, C.c_uint32, C.POINTER(MstEdge), u64, C.POINTER(u64), C.POINTER(MstNearest), C.POINTER(C.c_uint32)]
    L.bk_build_index.restype = C.c_int
    L.bk_build_index.argtypes = [i32, i32, vp, vp, vp, i32, C.POINTER(BuiltIndex)]
    L.bk_built_index_free.argtypes = [C.POINTER(BuiltIndex)]
    L.bk_build_last_error.restype = C.c_char_p
    L.bk_timing_enable.restype = C.c_int
    L.bk_timing_enable.argtypes = [vp, C.c_int]
    L.bk_timing_read.restype = C.c_int
    L.bk_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64), C.c_int]
    _libs[testing] = L
    return L
