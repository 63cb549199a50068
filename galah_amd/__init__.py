"""galah_amd -- MI355X-native finch MinHash precluster path for galah.

Python host mirror of the reference interface for this path, over the C ABI
of libgalahgpu.so (include/galahgpu.h):

  reference (AroneyS/galah @ 2024-12-18)              here
  src/lib.rs:23-27     trait PreclusterDistanceFinder  PreclusterDistanceFinder
  src/finch.rs:4-24    struct FinchPreclusterer        FinchPreclusterer
  src/finch.rs:26-75   finch::distances                distances()
  src/sorted_pair_genome_distance_cache.rs:4-59        SortedPairGenomeDistanceCache
  src/cluster_argument_parsing.rs:1160-1182            parse_percentage()
  src/genome_stats.rs:4-51                             GenomeAssemblyStats, calculate_genome_stats()
  src/cluster_validation.rs:7-78                       validate_clusters()
  src/cluster_validation.rs:80-113                     read_clustering_file()
  src/cluster_argument_parsing.rs:437-449, :478-484    write_cluster_definition(), write_representative_list()

There is no CPU fallback: importing works without a GPU (so the ABI can be
inspected), but every compute call needs a gfx950 device and raises
GalahGpuError otherwise.  The library must have been built in-tree
(`make -C galah_amd/csrc` or __graft_entry__.build()); a missing library is
an ImportError, never a silent substitute.

Every wrapper goes through one call frame: _tcall /
Context._call / Context._hcall turn a status into the exception of its error
source; _paths_arg, _dir_arg and _rows_out make the arguments; _PairsOut and
_take_array take what the library allocated.  This stays one file: the tests
execute it a second time as a plain module over a second library.
"""
import contextlib
import ctypes
import logging
import os

import numpy as np

__all__ = [
    "GalahGpuError", "Context", "Packed", "pack_files", "pack_records",
    "ani_f32", "ani_f64", "parse_percentage", "pair_tiles", "pair_partition",
    "SortedPairGenomeDistanceCache", "PreclusterDistanceFinder",
    "FinchPreclusterer", "distances", "PAIR_DTYPE", "LIB_PATH", "EXPORTED_SYMBOLS", "device_runs",
    "partition_preclusters", "precluster_pairs", "preclusters", "LOCAL_PAIR_DTYPE",
    "sketch_cache_load", "sketch_cache_store",
    "GenomeAssemblyStats", "calculate_genome_stats", "genome_stats", "STATS_DTYPE",
    "cluster_pairs_host", "clusters_from_reps", "ClusterDistanceFinder", "FinchClusterer", "cluster",
    "ani_pairs_host", "validate_clusters_host", "Validation", "ClusterValidation", "validate_clusters",
    "read_clustering_file", "write_cluster_definition", "write_representative_list",
    "pairs_border_host", "PreclusterState", "relabel_pairs", "cluster_update",
    "ani_matrix_host", "ani_matrix", "write_ani_matrix",
    "ani_matrix_group_cells", "ani_matrix_groups_host", "ani_matrix_block", "precluster_ani_matrices",
    "Collection", "query_host", "query_best_host",
]

HERE = os.path.dirname(os.path.abspath(__file__))
# GALAHGPU_LIB points at an alternate build (A/B kernel experiments)
LIB_PATH = os.environ.get("GALAHGPU_LIB") or os.path.join(HERE, "lib", "libgalahgpu.so")

GG_PAIR_TILE = 64  # include/galahgpu.h: pair tiles are 64 x 64
PAIR_DTYPE = np.dtype([("i", np.uint32), ("j", np.uint32), ("common", np.uint32), ("total", np.uint32)])

# every function include/galahgpu.h declares
EXPORTED_SYMBOLS = (
    "gg_abi_version", "gg_status_string", "gg_last_error", "gg_thread_last_error",
    "gg_create", "gg_destroy", "gg_device",
    "gg_pack_files", "gg_pack_records", "gg_packed_free",
    "gg_sketch", "gg_sketch_device",
    "gg_pair_tiles", "gg_pair_partition", "gg_pairs", "gg_pairs_device",
    "gg_precluster_files", "gg_ani_f64", "gg_ani_f32", "gg_parse_percentage",
    "gg_free", "gg_synth_clustered_device", "gg_timing_enable", "gg_timing_read", "gg_pair_paths",
    "gg_partition_preclusters", "gg_precluster_pairs", "gg_synth_mixed_lengths", "gg_synth_mixed_device",
    "gg_sketch_cache_load", "gg_sketch_cache_store", "gg_sketch_files", "gg_precluster_files_cached",
    "gg_create_multi", "gg_device_count", "gg_device_ctx", "gg_set_host_threads", "gg_phase_times",
    "gg_precluster_shards", "gg_fallbacks", "gg_peer_links", "gg_info_line", "gg_precluster_files_each",
    "gg_genome_stats_files", "gg_sketch_files_stats",
    "gg_cluster_pairs_host", "gg_cluster_pairs", "gg_cluster_pairs_device", "gg_clusters_from_reps", "gg_cluster_files",
    "gg_ani_pairs_host", "gg_ani_pairs", "gg_ani_pairs_device",
    "gg_validate_clusters_host", "gg_validate_clusters", "gg_validate_files",
    "gg_pairs_border", "gg_pairs_border_device", "gg_pairs_border_host", "gg_update_files",
    "gg_preclusters", "gg_preclusters_device",
    "gg_ani_f32_device", "gg_cluster_rows_device", "gg_cluster_files_resident",
    "gg_ani_matrix_host", "gg_ani_matrix", "gg_ani_matrix_device", "gg_ani_matrix_files",
    "gg_ani_matrix_group_cells", "gg_ani_matrix_groups_host", "gg_ani_matrix_groups", "gg_ani_matrix_groups_device",
    "gg_precluster_matrices_files",
    "gg_pairs_matrix_device", "gg_pairs_matrix", "gg_pairs_border_matrix_device", "gg_pairs_border_matrix",
    "gg_set_pairs_path", "gg_pairs_path", "gg_pairs_paths_taken",
    "gg_precluster_files_resident",
    "gg_collection_create", "gg_collection_destroy", "gg_collection_stat", "gg_collection_load",
    "gg_collection_add_rows", "gg_collection_add_rows_device", "gg_collection_add_files", "gg_collection_remove",
    "gg_collection_cluster", "gg_collection_pairs", "gg_collection_rows", "gg_collection_view",
    "gg_query_host", "gg_query_rows", "gg_query_rows_device", "gg_query_best_host", "gg_query_best_device",
    "gg_collection_query_rows", "gg_collection_query_files", "gg_collection_classify_rows",
    "gg_collection_classify_files",
)

GG_OK = 0
GG_ERR_NO_DEVICE = 4


class GalahGpuError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (status %d)" % (message, status))
        self.status = status


class _Run(ctypes.Structure):
    _fields_ = [("genome", ctypes.c_uint32), ("len", ctypes.c_uint32), ("base", ctypes.c_uint64)]


class _Shard(ctypes.Structure):
    _fields_ = [("d_words", ctypes.c_void_p), ("n_words", ctypes.c_uint64), ("runs", ctypes.c_void_p),
                ("n_runs", ctypes.c_uint64), ("n_genomes", ctypes.c_uint32)]


class _Packed(ctypes.Structure):
    _fields_ = [("words", ctypes.POINTER(ctypes.c_uint32)), ("n_words", ctypes.c_uint64),
                ("n_bases", ctypes.c_uint64), ("runs", ctypes.POINTER(_Run)), ("n_runs", ctypes.c_uint64),
                ("n_genomes", ctypes.c_uint32), ("genome_kmers", ctypes.POINTER(ctypes.c_uint64))]


RUN_DTYPE = np.dtype([("genome", np.uint32), ("len", np.uint32), ("base", np.uint64)])

# torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Load it
# first when it is installed so the process has ONE HIP runtime, shared by
# torch tensors/streams and libgalahgpu; loading ours first would make
# torch load a second runtime beside it.
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is optional for the ABI
    torch = None

if not os.path.exists(LIB_PATH):
    raise ImportError("libgalahgpu.so is not built (%s); run `make -C galah_amd/csrc` "
                      "or __graft_entry__.build()" % LIB_PATH)

_L = ctypes.CDLL(LIB_PATH)
_vp = ctypes.c_void_p
_u32, _u64, _i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
# the spellings the signature table repeats
_f32, _f64, _str, _byref = ctypes.c_float, ctypes.c_double, ctypes.c_char_p, ctypes.byref
_pvp, _pu32, _pu64, _pi32, _pstr = (ctypes.POINTER(t) for t in (_vp, _u32, _u64, _i32, _str))


def _sig(name, res, args):
    try:
        f = getattr(_L, name)
    except AttributeError:
        if "GALAHGPU_LIB" in os.environ:  # (an older build under A/B: its missing entry points stay unbound)
            return
        raise
    f.restype = res
    f.argtypes = args


class _Summary(ctypes.Structure):
    """A summary struct of counters: as_dict gives every field as an int (a `reserved` word is left out)."""

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_ if f != "reserved"}


_sig("gg_abi_version", _u32, [])
_sig("gg_status_string", _str, [_i32])
_sig("gg_last_error", _str, [_vp])
_sig("gg_thread_last_error", _str, [])
_sig("gg_create", _vp, [_i32, _u32, _u64, _i32, _pi32])
_sig("gg_destroy", None, [_vp])
_sig("gg_device", _i32, [_vp])
_sig("gg_create_multi", _vp, [_i32, _u32, _u64, _vp, _u32, _pi32])
_sig("gg_device_count", _u32, [_vp])
_sig("gg_device_ctx", _vp, [_vp, _u32])
_sig("gg_set_host_threads", _i32, [_vp, _i32])
_sig("gg_phase_times", _i32, [_vp, _vp])
_sig("gg_precluster_shards", _i32, [_vp, _vp, _f32, _pvp, _pvp, _pu64])
_sig("gg_pack_files", _i32, [_pstr, _u32, _i32, _i32, ctypes.POINTER(ctypes.POINTER(_Packed))])
_sig("gg_pack_records", _i32, [_pvp, _vp, _vp, _u64, _u32, _i32, ctypes.POINTER(ctypes.POINTER(_Packed))])
_sig("gg_packed_free", None, [ctypes.POINTER(_Packed)])
_sig("gg_sketch", _i32, [_vp, ctypes.POINTER(_Packed), _vp, _vp])
_sig("gg_sketch_device", _i32, [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _vp])
_sig("gg_pair_tiles", _u64, [_u32])
_sig("gg_pair_partition", None, [_u32, _u32, _u32, _pu64, _pu64])
_sig("gg_pairs", _i32, [_vp, _vp, _vp, _u32, _f32, _pvp, _pu64])
_sig("gg_pairs_device", _i32, [_vp, _vp, _vp, _u32, _u64, _u64, _f32, _vp, _u64, _vp, _vp])
_sig("gg_pairs_border", _i32, [_vp, _vp, _vp, _u32, _u32, _f32, _pvp, _pu64])
_sig("gg_pairs_border_device", _i32, [_vp, _vp, _vp, _u32, _u32, _f32, _vp, _u64, _vp, _vp])
_sig("gg_pairs_border_host", _i32, [_vp, _vp, _u32, _u32, _u32, _i32, _f32, _pvp, _pu64])
_sig("gg_update_files", _i32, [_vp, _vp, _vp, _u32, _pstr, _u32, _f32, _str, _vp, _vp, _pvp, _pvp, _pu64])
_sig("gg_precluster_files", _i32, [_vp, _pstr, _u32, _f32, _pvp, _pvp, _pu64])
_sig("gg_precluster_files_cached", _i32, [_vp, _pstr, _u32, _f32, _str, _pvp, _pvp, _pu64, _pu32])
# gg_pair_sink: int (*)(void* user, const gg_pair* pairs, uint64_t n)
PAIR_SINK = ctypes.CFUNCTYPE(_i32, _vp, _vp, _u64)
_sig("gg_precluster_files_each", _i32, [_vp, _pstr, _u32, _f32, _str, PAIR_SINK, _vp, _pvp, _pvp, _pu64, _pu32])
_sig("gg_sketch_files", _i32, [_vp, _pstr, _u32, _str, _vp, _vp, _pu32])
_sig("gg_genome_stats_files", _i32, [_pstr, _u32, _i32, _vp])
_sig("gg_sketch_files_stats", _i32, [_vp, _pstr, _u32, _str, _vp, _vp, _vp])
_sig("gg_sketch_cache_load", _i32, [_str, _str, _i32, _u32, _u64, _vp, _pu32, _pi32])
_sig("gg_sketch_cache_store", _i32, [_str, _str, _i32, _u32, _u64, _vp, _u32])
_sig("gg_ani_f64", _f64, [_u32, _u32, _i32])
_sig("gg_ani_f32", _f32, [_u32, _u32, _i32])
_sig("gg_parse_percentage", _i32, [_f32, ctypes.POINTER(_f32)])
_sig("gg_free", None, [_vp])
_sig("gg_synth_clustered_device", _i32, [_vp, _u32, _u32, _u32, _u32, _f32, _u64, _vp, _vp, _vp])
_sig("gg_synth_mixed_lengths", _i32, [_u32, _u32, _u32, _u32, _u32, _u64, _vp])
_sig("gg_synth_mixed_device", _i32, [_vp, _u32, _u32, _vp, _u32, _f32, _f64, _u64, _vp, _vp, _u64, _pu64, _vp])
_sig("gg_partition_preclusters", _i32, [_u32, _vp, _u64, _vp, _vp, _pu32])
_sig("gg_precluster_pairs", _i32, [_u32, _vp, _u64, _vp, _vp, _u32, _vp, _vp])
_sig("gg_preclusters", _i32, [_vp, _u32, _vp, _u64, _vp, _vp, _pu32, _vp, _vp])
_sig("gg_preclusters_device", _i32, [_vp, _u32, _vp, _u64, _vp, _vp, _pu32, _vp, _vp, _vp])
_sig("gg_cluster_pairs_host", _i32, [_u32, _vp, _vp, _u64, _f32, _vp])
_sig("gg_cluster_pairs", _i32, [_vp, _u32, _vp, _vp, _u64, _f32, _vp])
_sig("gg_cluster_pairs_device", _i32, [_vp, _u32, _vp, _vp, _u64, _f32, _vp, _vp])
_sig("gg_clusters_from_reps", _i32, [_u32, _vp, _vp, _vp, _pu32])
_sig("gg_cluster_files", _i32, [_vp, _pstr, _u32, _f32, _f32, _str, _vp, _pvp, _pvp, _pu64])


class _ClusterSummary(_Summary):
    _fields_ = [("n_pairs", ctypes.c_uint64), ("ani_rechecked", ctypes.c_uint64), ("n_preclusters", ctypes.c_uint32),
                ("largest_precluster", ctypes.c_uint32), ("pair_passes", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


_sig("gg_ani_f32_device", _i32, [_vp, _vp, _u64, _vp, _vp, _pu64, _vp])
_sig("gg_cluster_rows_device", _i32, [_vp, _vp, _vp, _u32, _f32, _f32, _vp, ctypes.POINTER(_ClusterSummary), _pvp, _pvp,
                                      _vp])
_sig("gg_cluster_files_resident", _i32, [_vp, _pstr, _u32, _f32, _f32, _str, _vp, ctypes.POINTER(_ClusterSummary)])
_sig("gg_ani_pairs_host", _i32, [_vp, _vp, _u32, _u32, _i32, _vp, _u64, _vp])
_sig("gg_ani_pairs", _i32, [_vp, _vp, _vp, _u32, _vp, _u64, _vp])
_sig("gg_ani_pairs_device", _i32, [_vp, _vp, _vp, _u32, _vp, _u64, _vp])


class _MatrixSummary(_Summary):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_columns", ctypes.c_uint64), ("column_entries", ctypes.c_uint64),
                ("ani_rechecked", ctypes.c_uint64)]


_pms = ctypes.POINTER(_MatrixSummary)
_sig("gg_ani_matrix_host", _i32, [_vp, _vp, _u32, _u32, _i32, _vp, _u32, _vp, _vp, _vp])
_sig("gg_ani_matrix", _i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _pms])
_sig("gg_ani_matrix_device", _i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _pms, _vp])
_sig("gg_ani_matrix_files", _i32, [_vp, _pstr, _u32, _str, _vp, _vp, _vp, _pms])
_sig("gg_ani_matrix_group_cells", _i32, [_vp, _u32, _vp])
_sig("gg_ani_matrix_groups_host", _i32, [_vp, _vp, _u32, _u32, _i32, _vp, _vp, _u32, _vp, _vp, _vp])
_sig("gg_ani_matrix_groups", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _pms])
_sig("gg_ani_matrix_groups_device", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _pms, _vp])
_sig("gg_precluster_matrices_files", _i32, [_vp, _pstr, _u32, _f32, _str, _pvp, _pvp, _pu32, _pvp, _pvp, _pvp, _pvp,
                                            _pms])


class _PairsMatrixSummary(_Summary):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_columns", ctypes.c_uint64), ("column_entries", ctypes.c_uint64),
                ("n_pairs", ctypes.c_uint64), ("chunk_rounds", ctypes.c_uint64), ("index_reads", ctypes.c_uint64),
                ("path", ctypes.c_uint32), ("pair_passes", ctypes.c_uint32)]

    def as_dict(self):
        d = super().as_dict()
        d["path"] = PAIRS_PATHS[d["path"]]
        return d


PAIRS_PATHS = ("default", "matrix", "auto")  # GG_PAIRS_PATH_*
_ppms = ctypes.POINTER(_PairsMatrixSummary)
_sig("gg_pairs_matrix_device", _i32, [_vp, _vp, _vp, _u32, _vp, _u32, _f32, _vp, _u64, _vp, _ppms, _vp])
_sig("gg_pairs_matrix", _i32, [_vp, _vp, _vp, _u32, _vp, _u32, _f32, _pvp, _pu64, _ppms])
_sig("gg_pairs_border_matrix_device", _i32, [_vp, _vp, _vp, _u32, _u32, _f32, _vp, _u64, _vp, _ppms, _vp])
_sig("gg_pairs_border_matrix", _i32, [_vp, _vp, _vp, _u32, _u32, _f32, _pvp, _pu64, _ppms])
_sig("gg_set_pairs_path", _i32, [_vp, _i32])
_sig("gg_pairs_path", _i32, [_vp])
_sig("gg_pairs_paths_taken", _i32, [_vp, _vp])
_sig("gg_precluster_files_resident", _i32, [_vp, _pstr, _u32, _f32, _str, _pvp, _pvp, _pu64, _ppms])


class _CollectionInfo(_Summary):
    _fields_ = [("n_pairs", ctypes.c_uint64), ("pair_capacity", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("n_rows", ctypes.c_uint32), ("row_capacity", ctypes.c_uint32), ("grows", ctypes.c_uint32),
                ("rows_moved", ctypes.c_uint32)]


_sig("gg_collection_create", _i32, [_vp, _f32, _u32, _u64, _pvp])
_sig("gg_collection_destroy", None, [_vp])
_sig("gg_collection_stat", _i32, [_vp, ctypes.POINTER(_CollectionInfo), ctypes.POINTER(_f32)])
_sig("gg_collection_load", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _f32, _pvp])
_sig("gg_collection_add_rows", _i32, [_vp, _vp, _vp, _u32, _pu64])
_sig("gg_collection_add_rows_device", _i32, [_vp, _vp, _vp, _u32, _pu64, _vp])
_sig("gg_collection_add_files", _i32, [_vp, _pstr, _u32, _str, _pu64])
_sig("gg_collection_remove", _i32, [_vp, _vp, _u32, _vp])
_sig("gg_collection_cluster", _i32, [_vp, _vp, _f32, _vp])
_sig("gg_collection_pairs", _i32, [_vp, _pvp, _pvp, _pu64])
_sig("gg_collection_rows", _i32, [_vp, _vp, _vp])
_sig("gg_collection_view", _i32, [_vp, _pvp, _pvp, _pvp, _pvp])
_sig("gg_query_host", _i32, [_vp, _vp, _u32, _vp, _vp, _u32, _u32, _i32, _f32, _pvp, _pu64])
_sig("gg_query_rows", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _f32, _pvp, _pvp, _pu64])
_sig("gg_query_rows_device", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _f32, _vp, _u64, _vp, _vp])
_sig("gg_query_best_host", _i32, [_u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp])
_sig("gg_query_best_device", _i32, [_vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp])
_sig("gg_collection_query_rows", _i32, [_vp, _vp, _vp, _u32, _f32, _pvp, _pvp, _pu64])
_sig("gg_collection_query_files", _i32, [_vp, _pstr, _u32, _str, _f32, _vp, _vp, _pvp, _pvp, _pu64])
_sig("gg_collection_classify_rows", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _vp])
_sig("gg_collection_classify_files", _i32, [_vp, _pstr, _u32, _str, _vp, _vp, _vp])


class _Validation(ctypes.Structure):
    _fields_ = [("member_pairs", ctypes.c_uint64), ("member_bad", ctypes.c_uint64), ("rep_pairs", ctypes.c_uint64),
                ("rep_bad", ctypes.c_uint64)]


_VOUT = [ctypes.POINTER(_Validation), _pvp, _pvp, _pu64]
_sig("gg_validate_clusters_host", _i32, [_vp, _vp, _u32, _u32, _i32, _vp, _vp, _u32, _f32] + _VOUT)
_sig("gg_validate_clusters", _i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _f32] + _VOUT)
_sig("gg_validate_files", _i32, [_vp, _pstr, _u32, _vp, _vp, _u32, _f32, _str] + _VOUT)


class _KStats(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double), ("launches", ctypes.c_uint64), ("work", ctypes.c_uint64)]


_sig("gg_timing_enable", _i32, [_vp, _i32])
_sig("gg_pair_paths", _i32, [_vp, _vp])
_sig("gg_fallbacks", _i32, [_vp, _vp])
_sig("gg_peer_links", _i32, [_vp, _vp])
_sig("gg_info_line", _i32, [_vp, _str, ctypes.c_size_t])
FALLBACKS = ("index_to_gate", "index_full_sort", "peer_staged", "sketch_retry", "inflate_host", "sketch_set")  # gg_fallbacks order
_sig("gg_timing_read", _i32, [_vp, _i32, ctypes.POINTER(_KStats)])
KERNEL_SKETCH, KERNEL_FINALIZE, KERNEL_PAIRS, KERNEL_PAIRS_INDEX = 0, 1, 2, 3
# the device-inflate ingest's kernels (gzip lists through precluster_files / sketch_files)
(KERNEL_INFLATE_SEARCH, KERNEL_INFLATE_DECODE, KERNEL_INFLATE_EXPAND, KERNEL_INFLATE_RESOLVE, KERNEL_INFLATE_CRC,
 KERNEL_PARSE, KERNEL_UPLOAD) = range(4, 11)
KERNEL_CLUSTER = 11  # every kernel of cluster_pairs / cluster_pairs_device (work: pairs)
KERNEL_ANI_PAIRS = 12  # the named-pair kernel of ani_pairs / ani_pairs_device / validate_clusters (work: listed pairs)
KERNEL_PRECLUSTER = 13  # every kernel of preclusters / preclusters_device (work: pairs)
INGEST_KERNELS = {"search": KERNEL_INFLATE_SEARCH, "decode": KERNEL_INFLATE_DECODE, "expand": KERNEL_INFLATE_EXPAND,
                  "resolve": KERNEL_INFLATE_RESOLVE, "crc": KERNEL_INFLATE_CRC, "parse": KERNEL_PARSE,
                  "upload": KERNEL_UPLOAD}


def lib():
    """The loaded ctypes handle of libgalahgpu.so."""
    return _L


def _ptr(a):
    return a.ctypes.data_as(_vp)


def _thread_err(st):
    return GalahGpuError(st, _L.gg_thread_last_error().decode(errors="replace"))


# ---------------------------------------------------------------------------
# The call frame
# ---------------------------------------------------------------------------
def _tcall(fn, *args):
    """fn(*args) of an entry point that reports on the calling thread (the
    host forms, and gg_collection_stat / gg_collection_view)."""
    st = fn(*args)
    if st != GG_OK:
        raise _thread_err(st)


def _paths_arg(paths):
    """(char* array, n) of a list of paths; the array has one entry at least."""
    n = len(paths)
    return (_str * max(n, 1))(*[os.fsencode(p) for p in paths]), n


def _dir_arg(cache_dir):
    """A sketch cache directory as the library takes it: None is NULL, "" is passed on."""
    return None if cache_dir is None else os.fsencode(cache_dir)


def _rows_out(n, s):
    """Row outputs for the library to fill -> (sketches pointer, lens pointer,
    sketches [n, s] u64, lens [n] u32): allocated for one row at least, the
    arrays returned are the first n rows of what the pointers name."""
    out, lens = np.zeros((max(n, 1), s), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
    return _ptr(out), _ptr(lens), out[:n], lens[:n]


def _best_out(nq):
    """The outputs of a best-candidate call, as _rows_out -> (best pointer, ani pointer, best [nq], best_ani [nq])."""
    best, best_ani = np.zeros(max(nq, 1), dtype=PAIR_DTYPE), np.zeros(max(nq, 1), dtype=np.float32)
    return _ptr(best), _ptr(best_ani), best[:nq], best_ani[:nq]


def _take_array(ptr, count, dtype):
    """An array the library allocated, as a fresh numpy array; the library's is released."""
    if count:
        # one memmove into a fresh array (a ctypes array type per call, or
        # np.ctypeslib.as_array, cost ~0.1-0.25 ms at C3's 15k pairs)
        out = np.empty(count, dtype=dtype)
        ctypes.memmove(out.ctypes.data, ptr.value, count * out.itemsize)
    else:
        out = np.zeros(0, dtype=dtype)
    _L.gg_free(ptr)
    return out


def _take_pairs(ptr, n):
    return _take_array(ptr, n, PAIR_DTYPE)


def _take_pairs_ani(pp, ap, n):
    ani = _take_array(ap, n, np.float32)
    return _take_pairs(pp, n), ani


class _PairsOut:
    """The (gg_pair*, float*, uint64_t) a call returns its pairs in (without
    ani: the pairs and their count alone): .refs are the arguments, take()
    gives (pairs, ani f32), or the pairs, and releases the library's arrays."""

    def __init__(self, ani=True):
        self.pp, self.ap, self.cnt = _vp(), (_vp() if ani else None), _u64()
        self.refs = tuple(_byref(x) for x in (self.pp, self.ap, self.cnt) if x is not None)

    def take(self):
        if self.ap is None:
            return _take_pairs(self.pp, self.cnt.value)
        return _take_pairs_ani(self.pp, self.ap, self.cnt.value)


def abi_version():
    return _L.gg_abi_version()


def ani_f64(common, total, k=21):
    """src/finch.rs:56-64: 1 - finch mash_distance (f64)."""
    return _L.gg_ani_f64(common, total, k)


def ani_f32(common, total, k=21):
    """The stored value, Some(ani as f32) (src/finch.rs:70)."""
    return np.float32(_L.gg_ani_f32(common, total, k))


def parse_percentage(value):
    """CAP:1160-1182 for --precluster-ani: [1,100] -> /100 in f32,
    [0,1) kept, anything else is an error."""
    out = _f32()
    st = _L.gg_parse_percentage(_f32(value), _byref(out))
    if st != GG_OK:  # (its own class and text: the reference's message, no status suffix)
        raise ValueError(_L.gg_thread_last_error().decode())
    return np.float32(out.value)


def pair_tiles(n):
    return _L.gg_pair_tiles(n)


def pair_partition(n, parts, part):
    b, e = _u64(), _u64()
    _L.gg_pair_partition(n, parts, part, _byref(b), _byref(e))
    return b.value, e.value


LOCAL_PAIR_DTYPE = np.dtype([("precluster", np.uint32), ("i", np.uint32), ("j", np.uint32), ("src", np.uint32)])


def _as_pairs(pairs):
    p = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    for f in ("i", "j"):
        p[f] = pairs[f]
    for f in ("common", "total"):
        if pairs.dtype.names and f in pairs.dtype.names:
            p[f] = pairs[f]
    return p


def synth_mixed_lengths(n_genomes, min_len, max_len, cluster_size, seed, first_genome=0):
    """Config C5 genome lengths: log-uniform in [min_len, max_len] per cluster."""
    lens = np.zeros(max(n_genomes, 1), np.uint32)
    _tcall(_L.gg_synth_mixed_lengths, first_genome, n_genomes, min_len, max_len, cluster_size, seed, _ptr(lens))
    return lens[:n_genomes]


def partition_preclusters(n_genomes, pairs):
    """src/clusterer.rs:409-431 partition_sketches + :45-57: single linkage
    over the passing pairs -> (members, offsets): precluster s is
    members[offsets[s]:offsets[s+1]], ascending; largest precluster first,
    ties by smallest member.  Host C++ (union-find), linear in the pairs."""
    p = _as_pairs(pairs)
    members = np.zeros(max(n_genomes, 1), np.uint32)
    offsets = np.zeros(n_genomes + 1, np.uint32)
    ns = _u32()
    _tcall(_L.gg_partition_preclusters, n_genomes, _ptr(p), len(p), _ptr(members), _ptr(offsets), _byref(ns))
    return members[:n_genomes], offsets[:ns.value + 1].copy()


def precluster_pairs(n_genomes, pairs, members, offsets):
    """transform_ids (src/sorted_pair_genome_distance_cache.rs:47-58) for
    every precluster at once -> (local pairs [LOCAL_PAIR_DTYPE] grouped by
    precluster and sorted by (i, j), pair_offsets)."""
    p = _as_pairs(pairs)
    members = np.ascontiguousarray(members, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    ns = len(offsets) - 1
    out = np.zeros(max(len(p), 1), LOCAL_PAIR_DTYPE)
    poff = np.zeros(ns + 1, np.uint64)
    _tcall(_L.gg_precluster_pairs, n_genomes, _ptr(p), len(p), _ptr(members), _ptr(offsets), ns, _ptr(out), _ptr(poff))
    return out[:len(p)], poff


def preclusters(n_genomes, pairs):
    """The preclusters as galah's cluster() holds them (src/clusterer.rs:45-57):
    a list of ascending index lists, largest first."""
    members, offsets = partition_preclusters(n_genomes, pairs)
    return [members[offsets[s]:offsets[s + 1]].tolist() for s in range(len(offsets) - 1)]


def _pairs_ani_arg(pairs, ani):
    """(PAIR_DTYPE array, f32 array) of a pair list and its ANI values: a
    structured array with i and j, or a sequence of (i, j) tuples."""
    if not (isinstance(pairs, np.ndarray) and pairs.dtype.names):
        ij = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
        pairs = np.zeros(len(ij), dtype=PAIR_DTYPE)
        pairs["i"], pairs["j"] = ij[:, 0], ij[:, 1]
    p = pairs if pairs.dtype == PAIR_DTYPE and pairs.flags.c_contiguous else _as_pairs(pairs)
    a = np.ascontiguousarray(ani, dtype=np.float32)
    if a.shape != (len(p),):
        raise ValueError("one ani per pair")
    return p, a


def cluster_pairs_host(n_genomes, pairs, ani, cluster_ani):
    """src/clusterer.rs:155-225 and :316-406 with the clusterer reusing the
    preclusterer's values (finch + finch), from the pair cache alone ->
    rep_of [n_genomes] u32 (rep_of[r] == r for a representative).  pairs in
    either orientation, any order; ani the f32 the cache stores for each.
    Host C++ (gg_cluster_pairs_host), linear in the pairs."""
    p, a = _pairs_ani_arg(pairs, ani)
    rep_of = np.zeros(max(n_genomes, 1), np.uint32)
    _tcall(_L.gg_cluster_pairs_host, n_genomes, _ptr(p), _ptr(a), len(p), _f32(cluster_ani), _ptr(rep_of))
    return rep_of[:n_genomes]


def clusters_from_reps(rep_of):
    """rep_of -> the clusters as lists of indices: by representative
    ascending, the representative first, then its members ascending."""
    rep_of = np.ascontiguousarray(rep_of, dtype=np.uint32)
    n = len(rep_of)
    members = np.zeros(max(n, 1), np.uint32)
    offsets = np.zeros(n + 1, np.uint32)
    nc = _u32()
    _tcall(_L.gg_clusters_from_reps, n, _ptr(rep_of), _ptr(members), _ptr(offsets), _byref(nc))
    return [members[offsets[c]:offsets[c + 1]].tolist() for c in range(nc.value)]


def _pair_list_arg(pairs):
    """A fresh PAIR_DTYPE array naming the pairs (common and total zero): from
    a structured array with i and j, or a sequence of (i, j)."""
    if isinstance(pairs, np.ndarray) and pairs.dtype.names:
        p = np.zeros(len(pairs), dtype=PAIR_DTYPE)
        p["i"], p["j"] = pairs["i"], pairs["j"]
        return p
    ij = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    p = np.zeros(len(ij), dtype=PAIR_DTYPE)
    p["i"], p["j"] = ij[:, 0], ij[:, 1]
    return p


def _rows_arg(sketches, lens, sketch_size=None):
    """(sketches [n, s] u64, lens [n] u32, n, s) of a sketch matrix."""
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    n = ln.shape[0]
    sk = np.ascontiguousarray(sketches, dtype=np.uint64)
    if n == 0:
        return sk, ln, 0, int(sketch_size or 1)
    if sk.ndim != 2 or sk.shape[0] != n or (sketch_size is not None and sk.shape[1] != sketch_size):
        raise ValueError("sketches must be [n, sketch_size]")
    return sk, ln, n, sk.shape[1]


def _clusters_arg(clusters):
    """(members u32, offsets u32, count) -- the CSR form of a list of index
    lists, each with its representative first."""
    sizes = [len(c) for c in clusters]
    offsets = np.zeros(len(sizes) + 1, np.uint32)
    np.cumsum(sizes, out=offsets[1:])
    members = np.zeros(max(int(offsets[-1]), 1), np.uint32)
    if offsets[-1]:
        members[:offsets[-1]] = np.concatenate([np.asarray(c, dtype=np.uint32).reshape(-1) for c in clusters])
    return members, offsets, len(sizes)


class Validation:
    """What validate_clusters found (src/cluster_validation.rs:7-78 with
    finch's ANI): the four counts of gg_validation, and the violations as
    PAIR_DTYPE records with their f32 ANI -- the members below the threshold
    as (representative, member), then the representatives at or above it as
    (r1 < r2)."""

    def __init__(self, summary, bad, bad_ani):
        self.member_pairs, self.member_bad = int(summary.member_pairs), int(summary.member_bad)
        self.rep_pairs, self.rep_bad = int(summary.rep_pairs), int(summary.rep_bad)
        self.bad, self.bad_ani = bad, bad_ani

    @property
    def ok(self):
        return self.member_bad == 0 and self.rep_bad == 0

    @property
    def member_violations(self):
        return self.bad[:self.member_bad], self.bad_ani[:self.member_bad]

    @property
    def rep_violations(self):
        return self.bad[self.member_bad:], self.bad_ani[self.member_bad:]

    def __repr__(self):
        return ("Validation(member_pairs=%d, member_bad=%d, rep_pairs=%d, rep_bad=%d)"
                % (self.member_pairs, self.member_bad, self.rep_pairs, self.rep_bad))


def ani_pairs_host(sketches, lens, pairs, k=21):
    """finch's merge counts and the stored f32 ANI of the pairs named
    (src/lib.rs:29-37 calculate_ani for a whole list; gg_ani_pairs_host, no
    device) -> (PAIR_DTYPE array in the order given, ani f32).  Either
    orientation, repeats and i == j are allowed; there is no threshold."""
    sk, ln, n, s = _rows_arg(sketches, lens)
    p = _pair_list_arg(pairs)
    ani = np.zeros(max(len(p), 1), np.float32)
    _tcall(_L.gg_ani_pairs_host, _ptr(sk), _ptr(ln), n, s, k, _ptr(p), len(p), _ptr(ani))
    return p, ani[:len(p)]


def _matrix_rows_arg(rows, n):
    """(rows u32 or None, its pointer, m) of a list of row indices; None: rows 0 .. n-1."""
    if rows is None:
        return None, None, n
    r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    return r, _ptr(r), len(r)


def _matrix_out(m):
    z = max(m, 1)
    return np.zeros((z, z), np.uint32), np.zeros((z, z), np.uint32), np.zeros((z, z), np.float32)


def ani_matrix_host(sketches, lens, rows=None, k=21):
    """The dense matrix of the rows listed (rows=None: all of them, in order):
    finch's merge counts and the stored f32 ANI of every two of them
    (gg_ani_matrix_host: the merge itself, no device) -> (common u32, total
    u32, ani f32), each [m, m].  Any order, a row may be listed more than
    once; the diagonal holds (len, len, 1.0), an empty row (0, 0, 0.0)."""
    sk, ln, n, s = _rows_arg(sketches, lens)
    r, rp, m = _matrix_rows_arg(rows, n)
    common, total, ani = _matrix_out(m)
    _tcall(_L.gg_ani_matrix_host, _ptr(sk), _ptr(ln), n, s, k, rp, m, _ptr(common), _ptr(total), _ptr(ani))
    return common[:m, :m], total[:m, :m], ani[:m, :m]


def _groups_arg(members, offsets):
    """(members u32, offsets u32, n_groups) of a CSR of groups; members may be
    a list of index lists (offsets None)."""
    if offsets is None:
        groups = [np.asarray(g, dtype=np.uint32).reshape(-1) for g in members]
        offsets = np.zeros(len(groups) + 1, np.uint32)
        if groups:
            offsets[1:] = np.cumsum([len(g) for g in groups])
        members = np.concatenate(groups) if groups else np.zeros(0, np.uint32)
    mem = np.ascontiguousarray(members, dtype=np.uint32).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    if len(off) < 1 or int(off[-1]) > len(mem):
        raise ValueError("offsets must have n_groups + 1 entries and end within members")
    return (mem if len(mem) else np.zeros(1, np.uint32)), off, len(off) - 1


def ani_matrix_group_cells(offsets):
    """cell_offsets [n_groups + 1] u64 of a CSR's offsets: block g of a
    grouped matrix call begins at cell_offsets[g] and holds m_g^2 cells
    (gg_ani_matrix_group_cells; raises for offsets that do not ascend from 0
    and for a call past the limits: 2^32 cells, 2^31 tile pairs)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    cells = np.zeros(len(off), np.uint64)
    _tcall(_L.gg_ani_matrix_group_cells, _ptr(off), len(off) - 1, _ptr(cells))
    return cells


def ani_matrix_block(values, offsets, cell_offsets, g):
    """Block g of a flat array of a grouped matrix call as an [m_g, m_g] view."""
    m = int(offsets[g + 1]) - int(offsets[g])
    return values[int(cell_offsets[g]):int(cell_offsets[g]) + m * m].reshape(m, m)


def _groups_out(members, offsets):
    """(members, offsets, n_groups, cell_offsets, common, total, ani) of a
    grouped matrix call: the flat outputs hold one cell at least, z =
    cell_offsets[-1] of them are the result."""
    mem, off, ng = _groups_arg(members, offsets)
    cells = ani_matrix_group_cells(off)
    z = max(int(cells[-1]), 1)
    return mem, off, ng, cells, np.zeros(z, np.uint32), np.zeros(z, np.uint32), np.zeros(z, np.float32)


def ani_matrix_groups_host(sketches, lens, members, offsets=None, k=21):
    """ani_matrix_host for every group of a CSR at once (group g is
    members[offsets[g]:offsets[g + 1]]; or members a list of index lists):
    gg_ani_matrix_groups_host, the merge itself, no device -> (common u32,
    total u32, ani f32, cell_offsets u64): flat arrays, block g row-major
    [m_g, m_g] at cell_offsets[g] (ani_matrix_block)."""
    sk, ln, n, s = _rows_arg(sketches, lens)
    mem, off, ng, cells, common, total, ani = _groups_out(members, offsets)
    _tcall(_L.gg_ani_matrix_groups_host, _ptr(sk), _ptr(ln), n, s, k, _ptr(mem), _ptr(off), ng, _ptr(common),
           _ptr(total), _ptr(ani))
    z = int(cells[-1])
    return common[:z], total[:z], ani[:z], cells


def pairs_border_host(sketches, lens, n_old, min_ani, k=21):
    """The border of a sketch matrix on the host (gg_pairs_border_host, no
    device): every passing pair (i < j) with j >= n_old, sorted by (i, j), so
    that pairs(rows) == pairs(rows[:n_old]) + pairs_border(rows, n_old) as
    sets.  n_old == 0 gives every pair, n_old == n none."""
    sk, ln, n, s = _rows_arg(sketches, lens)
    out = _PairsOut(ani=False)
    _tcall(_L.gg_pairs_border_host, _ptr(sk), _ptr(ln), n, int(n_old), s, int(k), _f32(min_ani), *out.refs)
    return out.take()


def query_host(sketches, lens, q_sketches, q_lens, min_ani, k=21):
    """The hits of queries against rows on the host (gg_query_host): every
    cell (row i, query q) that passes at min_ani as pair (i, n + q, common,
    total), sorted by (i, j); no query x query cell."""
    widths = [a.shape[1] for a in (np.asarray(sketches), np.asarray(q_sketches)) if a.ndim == 2 and a.shape[0]]
    s = int(widths[0]) if widths else 1  # (an empty side has no width of its own)
    sk, ln, n, _ = _rows_arg(sketches, lens, s)
    qs, ql, nq, _ = _rows_arg(q_sketches, q_lens, s)
    out = _PairsOut(ani=False)
    _tcall(_L.gg_query_host, _ptr(sk), _ptr(ln), n, _ptr(qs), _ptr(ql), nq, s, int(k), _f32(min_ani), *out.refs)
    return out.take()


def _rank_arg(rank, n):
    """(rank [n] u32 or None, its pointer) of a query's candidate ranks; None,
    or no rows: NULL, every row a candidate by its index."""
    if rank is None:
        return None, None
    rank = np.ascontiguousarray(rank, dtype=np.uint32).reshape(-1)
    if len(rank) != n:
        raise ValueError("one rank per row")
    return rank, (_ptr(rank) if n else None)


def query_best_host(n, nq, pairs, ani, rank=None):
    """Every query's best candidate (gg_query_best_host) -> (best [nq] pairs,
    i = 0xFFFFFFFF without a candidate hit; best_ani [nq] f32).  rank [n] u32,
    0xFFFFFFFF: no candidate; None: every row, by its index."""
    pa, an = _pairs_ani_arg(pairs, ani)
    rank, rp = _rank_arg(rank, n)
    bp, bap, best, best_ani = _best_out(nq)
    _tcall(_L.gg_query_best_host, int(n), int(nq), _ptr(pa) if len(pa) else None, _ptr(an) if len(an) else None,
           len(pa), rp, bp, bap)
    return best, best_ani


def validate_clusters_host(sketches, lens, clusters, ani, k=21):
    """src/cluster_validation.rs:7-78 over sketches (gg_validate_clusters_host,
    no device): clusters a list of index lists, each with its representative
    first; ani the threshold as an f32 fraction -> Validation."""
    sk, ln, n, s = _rows_arg(sketches, lens)
    members, offsets, nc = _clusters_arg(clusters)
    summary, bad = _Validation(), _PairsOut()
    _tcall(_L.gg_validate_clusters_host, _ptr(sk), _ptr(ln), n, s, k, _ptr(members), _ptr(offsets), nc, _f32(ani),
           _byref(summary), *bad.refs)
    return Validation(summary, *bad.take())


def read_clustering_file(path):
    """src/cluster_validation.rs:80-113: a cluster definition file (as
    write_cluster_definition, galah or dRep write it) -> the clusters as lists
    of path strings, each with its representative first.  Tab-separated,
    exactly two fields per line (ValueError otherwise); a line whose two
    fields are equal opens a cluster; lines before the first such line are
    dropped; a member line's first field is not compared with the open
    representative; empty lines are skipped.  Unlike the reference's csv
    reader, CSV quoting is not interpreted: a '"' is an ordinary byte."""
    clusters, current, have_rep = [], [], False
    with open(path, "r", encoding="utf-8", errors="surrogateescape", newline="") as f:
        text = f.read()
    for line in text.replace("\r\n", "\n").replace("\r", "\n").split("\n"):
        if line == "":
            continue
        fields = line.split("\t")
        if len(fields) != 2:
            raise ValueError("Unexpectedly didn't find exactly 2 fields in clustering file: StringRecord([%s])"
                             % ", ".join(_rust_str_debug(x) for x in fields))
        if fields[0] == fields[1]:
            if have_rep:
                clusters.append(current)
            current, have_rep = [], True
        current.append(fields[1])
    if have_rep:
        clusters.append(current)
    return clusters


def _rust_str_debug(x):
    return '"%s"' % x.replace("\\", "\\\\").replace('"', '\\"')


def _write_lines(f, lines):
    import io
    if isinstance(f, (str, bytes, os.PathLike)):
        with open(f, "wb") as g:
            _write_lines(g, lines)
        return
    binary = isinstance(f, (io.RawIOBase, io.BufferedIOBase))
    for line in lines:
        f.write(os.fsencode(line) if binary else line)


def write_cluster_definition(f, clusters, genomes):
    """src/cluster_argument_parsing.rs:437-449 (--output-cluster-definition):
    for every cluster, for every genome of it (the representative first, as
    itself), "<representative>\\t<genome>\\n".  clusters: lists of indices into
    genomes; f: a file object (text or binary) or a path."""
    _write_lines(f, ("%s\t%s\n" % (genomes[c[0]], genomes[g]) for c in clusters for g in c))


def write_representative_list(f, clusters, genomes):
    """src/cluster_argument_parsing.rs:478-484 (--output-representative-list):
    every cluster's representative, one per line."""
    _write_lines(f, ("%s\n" % genomes[c[0]] for c in clusters))


def sketch_cache_load(cache_dir, path, k=21, s=1000, seed=0):
    """the cached bottom-s sketch of a genome file
    (ascending u64 array), or None when there is no valid entry.  Host only."""
    out = np.zeros(max(int(s), 1), dtype=np.uint64)
    n, hit = _u32(), _i32()
    _tcall(_L.gg_sketch_cache_load, os.fsencode(cache_dir), os.fsencode(path), int(k), int(s), int(seed), _ptr(out),
           _byref(n), _byref(hit))
    return out[:n.value].copy() if hit.value else None


def sketch_cache_store(cache_dir, path, hashes, k=21, s=1000, seed=0):
    """Store the sketch of a genome file (strictly ascending, len <= s).  Host only."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64)
    _tcall(_L.gg_sketch_cache_store, os.fsencode(cache_dir), os.fsencode(path), int(k), int(s), int(seed), _ptr(h),
           len(h))


# gg_genome_stats
STATS_DTYPE = np.dtype([("num_contigs", np.uint64), ("num_ambiguous_bases", np.uint64), ("n50", np.uint64),
                        ("total_bases", np.uint64)])


class GenomeAssemblyStats:
    """src/genome_stats.rs:4-9: num_contigs, num_ambiguous_bases, n50
    (#[derive(Debug, PartialEq)] over those three).  total_bases, which the
    reference computes and drops, rides along outside equality and repr."""

    __slots__ = ("num_contigs", "num_ambiguous_bases", "n50", "total_bases")

    def __init__(self, num_contigs, num_ambiguous_bases, n50, total_bases=None):
        self.num_contigs = int(num_contigs)
        self.num_ambiguous_bases = int(num_ambiguous_bases)
        self.n50 = int(n50)
        self.total_bases = None if total_bases is None else int(total_bases)

    def _key(self):
        return (self.num_contigs, self.num_ambiguous_bases, self.n50)

    def __eq__(self, other):
        if not isinstance(other, GenomeAssemblyStats):
            return NotImplemented
        return self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "GenomeAssemblyStats { num_contigs: %d, num_ambiguous_bases: %d, n50: %d }" % self._key()


def _stats_list(arr):
    return [GenomeAssemblyStats(int(r["num_contigs"]), int(r["num_ambiguous_bases"]), int(r["n50"]),
                                int(r["total_bases"])) for r in arr]


def genome_stats(paths, threads=0):
    """src/genome_stats.rs:11 for every file, on `threads` host threads (0:
    the default of pack_files) -> a list of GenomeAssemblyStats.  Host only."""
    arr, n = _paths_arg(paths)
    out = np.zeros(max(n, 1), dtype=STATS_DTYPE)
    _tcall(_L.gg_genome_stats_files, arr, n, int(threads), _ptr(out))
    return _stats_list(out[:n])


def calculate_genome_stats(fasta_path):
    """src/genome_stats.rs:11-51 (a file that does not read or parse raises,
    where the reference panics)."""
    return genome_stats([fasta_path], threads=1)[0]


class Packed:
    """2-bit packed genomes (gg_packed), owned by the library."""

    def __init__(self, ptr):
        self._p = ptr
        self._free = _L.gg_packed_free  # kept: module globals may be gone at interpreter shutdown
        p = ptr.contents
        self.n_words = p.n_words
        self.n_bases = p.n_bases
        self.n_runs = p.n_runs
        self.n_genomes = p.n_genomes
        self.words = np.ctypeslib.as_array(p.words, shape=(max(p.n_words, 1),))[:p.n_words]
        runs_buf = (ctypes.c_char * (max(p.n_runs, 1) * RUN_DTYPE.itemsize)).from_address(
            ctypes.addressof(p.runs.contents))
        self.runs = np.frombuffer(runs_buf, dtype=RUN_DTYPE)[:p.n_runs]
        self.genome_kmers = np.ctypeslib.as_array(p.genome_kmers, shape=(max(p.n_genomes, 1),))[:p.n_genomes]

    def free(self):
        if self._p:
            self._free(self._p)
            self._p = None

    def __del__(self):
        self.free()


def pack_files(paths, k=21, threads=0):
    arr = (_str * len(paths))(*[os.fsencode(p) for p in paths])  # (no entry for no path: not _paths_arg's array)
    out = ctypes.POINTER(_Packed)()
    _tcall(_L.gg_pack_files, arr, len(paths), k, threads, _byref(out))
    return Packed(out)


def pack_records(genomes, k=21):
    """genomes: list (per genome) of lists of record byte strings."""
    recs, gid = [], []
    for g, rs in enumerate(genomes):
        for r in rs:
            recs.append(bytes(r))
            gid.append(g)
    bufs = [ctypes.create_string_buffer(r, len(r) + 1) for r in recs]
    seqs = (_vp * max(len(recs), 1))(*[ctypes.cast(b, _vp) for b in bufs])
    lens = np.array([len(r) for r in recs] or [0], dtype=np.uint64)
    gids = np.array(gid or [0], dtype=np.uint32)
    out = ctypes.POINTER(_Packed)()
    _tcall(_L.gg_pack_records, seqs, _ptr(lens), _ptr(gids), len(recs), len(genomes), k, _byref(out))
    return Packed(out)


def _dev_ptr(t):
    """Device pointer of a torch tensor or an int."""
    return t if isinstance(t, int) else t.data_ptr()


def _dev_opt(t):
    """_dev_ptr of an optional buffer: None is NULL."""
    return None if t is None else _dev_ptr(t)


def device_runs(runs, device):
    """A run table (RUN_DTYPE records) copied to a device tensor of 16-byte
    records, for sketch_device / precluster_shards to read in place."""
    runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
    return torch.from_numpy(runs.view(np.uint8).copy()).to(device)


def _runs_arg(runs):
    """(pointer, count, object to keep alive) of a run table: a RUN_DTYPE
    array (host memory) or a device tensor of 16-byte records."""
    if hasattr(runs, "data_ptr") and getattr(runs, "is_cuda", False):
        nbytes = runs.numel() * runs.element_size()
        if nbytes % RUN_DTYPE.itemsize or not runs.is_contiguous():
            raise ValueError("device run table: contiguous 16-byte records")
        return (runs.data_ptr() if nbytes else None), nbytes // RUN_DTYPE.itemsize, runs
    if hasattr(runs, "data_ptr"):  # a host torch tensor of 16-byte records (device_runs(..., "cpu"))
        nbytes = runs.numel() * runs.element_size()
        if nbytes % RUN_DTYPE.itemsize:
            raise ValueError("host run table tensor: 16-byte records")
        runs = runs.contiguous().numpy().view(np.uint8).reshape(-1).view(RUN_DTYPE)
        return runs.ctypes.data, len(runs), runs
    if not (isinstance(runs, np.ndarray) and runs.dtype == RUN_DTYPE):
        raise TypeError("run table: a RUN_DTYPE array or a device tensor of 16-byte records")
    runs = np.ascontiguousarray(runs)
    return runs.ctypes.data, len(runs), runs


PHASES = ("sketch", "replicate", "pairs", "merge")  # gg_phase_times order


class Context:
    """A gg_ctx: fixed k / sketch size / seed on one HIP device (device=...),
    or on several (devices=[...] ordinals, repeats allowed; devices="all":
    every visible device, or GALAHGPU_DEVICES when set)."""

    def __init__(self, k=21, sketch_size=1000, seed=0, device=-1, devices=None, host_threads=0):
        st = _i32()
        if devices is None:
            self._c = _L.gg_create(k, sketch_size, seed, device, _byref(st))
        elif devices == "all":
            self._c = _L.gg_create_multi(k, sketch_size, seed, None, 0, _byref(st))
        else:
            arr = (ctypes.c_int * max(len(devices), 1))(*devices)
            self._c = _L.gg_create_multi(k, sketch_size, seed, arr, len(devices), _byref(st))
        if not self._c:
            raise _thread_err(st.value)
        self.k, self.s, self.seed = k, sketch_size, seed
        # held by the instance: module globals may already be None when a
        # Context is collected at interpreter shutdown
        self._destroy = _L.gg_destroy
        if host_threads:
            self.set_host_threads(host_threads)

    def close(self):
        if getattr(self, "_c", None):
            self._destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _err(self, st):
        return GalahGpuError(st, _L.gg_last_error(self._c).decode(errors="replace"))

    def _hcall(self, fn, handle, *args):
        """fn(handle, *args) of an entry point that reports on this context:
        the gg_collection_* calls on a collection's handle."""
        st = fn(handle, *args)
        if st != GG_OK:
            raise self._err(st)

    def _call(self, fn, *args):
        """fn(this context, *args)."""
        self._hcall(fn, self._c, *args)

    _pairs_ani = staticmethod(_take_pairs_ani)

    @property
    def device(self):
        return _L.gg_device(self._c)

    @property
    def device_count(self):
        return _L.gg_device_count(self._c)

    def member(self, i):
        """Member i as a borrowed single-device handle (device-resident calls
        on that member's device); valid while this Context lives."""
        p = _L.gg_device_ctx(self._c, i)
        if not p:
            raise IndexError(i)
        m = Context.__new__(Context)
        m._c, m.k, m.s, m.seed = p, self.k, self.s, self.seed
        m._destroy = lambda _p: None  # owned by self
        m._owner = self
        return m

    def set_host_threads(self, n):
        """galah --threads (CAP:1327-1332): host threads for file ingest (<= 0: default)."""
        self._call(_L.gg_set_host_threads, int(n))

    def _counters(self, fn, count, dtype=np.uint64):
        """A read-out's array of `count` counters."""
        out = np.zeros(count, dtype)
        self._call(fn, _ptr(out))
        return out

    def phase_times(self):
        """Wall-clock ms of the last fused call's phases (PHASES)."""
        return dict(zip(PHASES, self._counters(_L.gg_phase_times, len(PHASES), np.float64).tolist()))

    def precluster_shards(self, shards, min_ani):
        """shards: one (d_words tensor, runs, n_genomes) per member,
        device-resident on that member's device (runs: a RUN_DTYPE array, or
        a device tensor holding the same 16-byte records, see device_runs)
        -> (pairs sorted by (i, j), ani f32), genomes numbered shard after
        shard."""
        if len(shards) != self.device_count:
            raise ValueError("one shard per device")
        keep = []
        arr = (_Shard * len(shards))()
        for x, (d_words, runs, ng) in enumerate(shards):
            rp, nr, runs = _runs_arg(runs)
            keep.append(runs)
            arr[x].d_words = _dev_ptr(d_words)
            arr[x].n_words = d_words.numel()
            arr[x].runs = rp
            arr[x].n_runs = nr
            arr[x].n_genomes = int(ng)
        out = _PairsOut()
        self._call(_L.gg_precluster_shards, arr, _f32(min_ani), *out.refs)
        return out.take()

    def timing_enable(self, on=True):
        self._call(_L.gg_timing_enable, 1 if on else 0)

    def pair_paths(self):
        """Which pair kernel ran, counted since the context was created
        (gg_pair_paths): {"index", "index_abandoned", "gate", "other",
        "index_full_sort"} ("index_full_sort" counts the index calls that
        used the full sort instead of the bucketed build)."""
        out = self._counters(_L.gg_pair_paths, 5)
        return dict(zip(("index", "index_abandoned", "gate", "other", "index_full_sort"), (int(x) for x in out)))

    def fallbacks(self):
        """Slow paths taken since the context was created (gg_fallbacks):
        {"index_to_gate", "index_full_sort", "peer_staged", "sketch_retry", "inflate_host", "sketch_set"}."""
        return dict(zip(FALLBACKS, (int(x) for x in self._counters(_L.gg_fallbacks, len(FALLBACKS)))))

    def peer_links(self):
        """[M, M] int array (gg_peer_links): 1 = member a copies from member b
        device to device, 0 = staged through host memory."""
        M = self.device_count
        return self._counters(_L.gg_peer_links, M * M, np.int32).reshape(M, M)

    def info_line(self):
        """The one-line summary galah would log at info! after distances()."""
        buf = ctypes.create_string_buffer(1024)
        self._call(_L.gg_info_line, buf, len(buf))
        return buf.value.decode()

    def timing_read(self, kernel):
        """-> dict(ms, launches, work) summed since timing_enable."""
        k = _KStats()
        self._call(_L.gg_timing_read, kernel, _byref(k))
        return {"ms": k.ms, "launches": k.launches, "work": k.work}

    # -- host-buffer API -------------------------------------------------
    def sketch(self, packed):
        """-> (sketches [n_genomes, s] u64 padded with 0, lens [n] u32)."""
        op, lp, out, lens = _rows_out(packed.n_genomes, self.s)
        self._call(_L.gg_sketch, packed._p, op, lp)
        return out, lens

    def pairs(self, sketches, lens, min_ani):
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        out = _PairsOut(ani=False)
        self._call(_L.gg_pairs, _ptr(sk), _ptr(ln), n, _f32(min_ani), *out.refs)
        return out.take()

    def pairs_border(self, sketches, lens, n_old, min_ani):
        """The border of a sketch matrix (gg_pairs_border): the passing pairs
        (i < j) with j >= n_old, sorted by (i, j) -- what rows [n_old, n) add
        to pairs(sketches[:n_old]).  On the context's (first) device; only the
        new rows are evaluated."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        out = _PairsOut(ani=False)
        self._call(_L.gg_pairs_border, _ptr(sk), _ptr(ln), n, int(n_old), _f32(min_ani), *out.refs)
        return out.take()

    def update_files(self, old_sketches, old_lens, new_paths, min_ani, cache_dir=None):
        """A finished run carried forward (gg_update_files): only new_paths are
        read and sketched (cache_dir as sketch_files), placed after the old
        rows, and the border evaluated -> (new sketches [n_new, s], new lens,
        border pairs sorted by (i, j) with indices into old + new, their f32
        ANI)."""
        sk, ln, n_old, _ = _rows_arg(old_sketches, old_lens, self.s)
        arr, n_new = _paths_arg(new_paths)
        op, lp, out, lens = _rows_out(n_new, self.s)
        border = _PairsOut()
        self._call(_L.gg_update_files, _ptr(sk), _ptr(ln), n_old, arr, n_new, _f32(min_ani), _dir_arg(cache_dir), op, lp,
                   *border.refs)
        pairs, ani = border.take()
        return out, lens, pairs, ani

    # ---- a collection resident on the device (gg_collection_*; class Collection wraps a handle)
    def collection_create(self, min_ani, reserve_rows=0, reserve_pairs=0):
        """An empty resident collection at min_ani -> its handle (collection_destroy frees it)."""
        h = _vp()
        self._call(_L.gg_collection_create, _f32(min_ani), int(reserve_rows), int(reserve_pairs), _byref(h))
        return h.value

    def collection_load(self, sketches, lens, pairs, ani, min_ani):
        """A collection from saved rows, pairs sorted by (i, j) and their f32
        ANI (checked for form, not recomputed) -> its handle."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        pa = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE).reshape(-1)
        an = np.ascontiguousarray(ani, dtype=np.float32).reshape(-1)
        if len(pa) != len(an):
            raise ValueError("one ANI value per pair")
        h = _vp()
        self._call(_L.gg_collection_load, _ptr(sk), _ptr(ln), n, _ptr(pa), _ptr(an), len(pa), _f32(min_ani), _byref(h))
        return h.value

    def collection_destroy(self, handle):
        _L.gg_collection_destroy(handle)

    def collection_stat(self, handle):
        """-> ({n_pairs, pair_capacity, device_bytes, n_rows, row_capacity, grows, rows_moved}, min_ani f32)."""
        info, thr = _CollectionInfo(), _f32()
        _tcall(_L.gg_collection_stat, handle, _byref(info), _byref(thr))  # (reports on the thread)
        return info.as_dict(), np.float32(thr.value)

    def _n_rows(self, handle):
        return self.collection_stat(handle)[0]["n_rows"]

    def collection_add_rows(self, handle, sketches, lens):
        """Host rows appended -> the number of border pairs added."""
        sk, ln, n_new, _ = _rows_arg(sketches, lens, self.s)
        added = _u64()
        self._hcall(_L.gg_collection_add_rows, handle, _ptr(sk), _ptr(ln), n_new, _byref(added))
        return added.value

    def collection_add_rows_device(self, handle, d_sketches, d_lens, n_new, stream=None):
        """Device rows (tensors or pointers) appended -> the number of border pairs added."""
        added = _u64()
        self._hcall(_L.gg_collection_add_rows_device, handle, _dev_ptr(d_sketches), _dev_ptr(d_lens), int(n_new),
                    _byref(added), stream)
        return added.value

    def collection_add_files(self, handle, paths, cache_dir=None):
        """Files sketched (cache_dir as sketch_files) and appended -> the number of border pairs added."""
        arr, n_new = _paths_arg(paths)
        added = _u64()
        self._hcall(_L.gg_collection_add_files, handle, arr, n_new, _dir_arg(cache_dir), _byref(added))
        return added.value

    def collection_remove(self, handle, rows):
        """Rows (any order, repeats allowed) removed -> new_index [n before]
        u32, 0xFFFFFFFF for a removed row."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        n = self._n_rows(handle)
        new_index = np.zeros(max(n, 1), np.uint32)
        self._hcall(_L.gg_collection_remove, handle, _ptr(rows) if len(rows) else None, len(rows), _ptr(new_index))
        return new_index[:n]

    def collection_cluster(self, handle, cluster_ani, order=None):
        """rep_of [n] u32 (positions in order; order: position -> row, None: identity)."""
        n = self._n_rows(handle)
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
            if len(order) != n:
                raise ValueError("order must be a permutation of 0 .. %d" % (n - 1))
        rep_of = np.zeros(max(n, 1), np.uint32)
        self._hcall(_L.gg_collection_cluster, handle, None if order is None or n == 0 else _ptr(order),
                    _f32(cluster_ani), _ptr(rep_of))
        return rep_of[:n]

    def collection_pairs(self, handle):
        """-> (pairs sorted by (i, j), ani f32)."""
        out = _PairsOut()
        self._hcall(_L.gg_collection_pairs, handle, *out.refs)
        return out.take()

    def collection_rows(self, handle):
        """-> (sketches [n, s] u64, lens [n] u32)."""
        op, lp, out, lens = _rows_out(self._n_rows(handle), self.s)
        self._hcall(_L.gg_collection_rows, handle, op, lp)
        return out, lens

    def collection_view(self, handle):
        """Device pointers (ints) of the sketches, lens, pairs and ANI, valid
        until the next call that changes the collection."""
        p = [_vp(), _vp(), _vp(), _vp()]
        _tcall(_L.gg_collection_view, handle, *[_byref(x) for x in p])  # (reports on the thread)
        return tuple(x.value or 0 for x in p)

    # ---- the query: hits and nearest representative of genomes that are not added (gg_query_*)
    def query_rows(self, sketches, lens, q_sketches, q_lens, min_ani):
        """-> (pairs (i, n + q, common, total) sorted by (i, j), ani f32) of
        the cells (row i, query q) that pass at min_ani."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        qs, ql, nq, _ = _rows_arg(q_sketches, q_lens, self.s)
        out = _PairsOut()
        self._call(_L.gg_query_rows, _ptr(sk), _ptr(ln), n, _ptr(qs), _ptr(ql), nq, _f32(min_ani), *out.refs)
        return out.take()

    def query_rows_device(self, d_sketches, d_lens, n, d_q_sketches, d_q_lens, nq, min_ani, d_out, out_cap, d_count,
                          stream=None):
        """Device rows and queries (tensors or pointers): the passing cells
        appended to d_out by pairs_device's output contract."""
        self._call(_L.gg_query_rows_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), int(n), _dev_ptr(d_q_sketches),
                   _dev_ptr(d_q_lens), int(nq), _f32(min_ani), _dev_opt(d_out), int(out_cap), _dev_ptr(d_count), stream)

    def query_best_device(self, n, nq, d_pairs, d_ani, n_pairs, d_rank, d_best, d_best_ani, stream=None):
        """Every query's best candidate from device hits (any order); d_rank may be None."""
        self._call(_L.gg_query_best_device, int(n), int(nq), _dev_ptr(d_pairs), _dev_ptr(d_ani), int(n_pairs),
                   _dev_opt(d_rank), _dev_ptr(d_best), _dev_ptr(d_best_ani), stream)

    def collection_query_rows(self, handle, q_sketches, q_lens, min_ani):
        """Host queries against a collection (unchanged by it) -> (pairs, ani)."""
        qs, ql, nq, _ = _rows_arg(q_sketches, q_lens, self.s)
        out = _PairsOut()
        self._hcall(_L.gg_collection_query_rows, handle, _ptr(qs), _ptr(ql), nq, _f32(min_ani), *out.refs)
        return out.take()

    def collection_query_files(self, handle, paths, min_ani, cache_dir=None, want_sketches=False):
        """Files sketched (cache_dir as sketch_files) and queried -> (pairs,
        ani), or (pairs, ani, sketches [nq, s], lens [nq]) with want_sketches."""
        arr, nq = _paths_arg(paths)
        op, lp, sk, lens = _rows_out(nq, self.s) if want_sketches else (None, None, None, None)
        out = _PairsOut()
        self._hcall(_L.gg_collection_query_files, handle, arr, nq, _dir_arg(cache_dir), _f32(min_ani), op, lp, *out.refs)
        pairs, ani = out.take()
        return (pairs, ani, sk, lens) if want_sketches else (pairs, ani)

    def collection_classify_rows(self, handle, q_sketches, q_lens, rank=None):
        """Every host query's best candidate at the collection's min_ani -> (best [nq], best_ani [nq])."""
        qs, ql, nq, _ = _rows_arg(q_sketches, q_lens, self.s)
        rank, rp = _rank_arg(rank, self._n_rows(handle))
        bp, bap, best, best_ani = _best_out(nq)
        self._hcall(_L.gg_collection_classify_rows, handle, _ptr(qs), _ptr(ql), nq, rp, bp, bap)
        return best, best_ani

    def collection_classify_files(self, handle, paths, rank=None, cache_dir=None):
        """Every file's best candidate at the collection's min_ani -> (best [nq], best_ani [nq])."""
        arr, nq = _paths_arg(paths)
        rank, rp = _rank_arg(rank, self._n_rows(handle))
        bp, bap, best, best_ani = _best_out(nq)
        self._hcall(_L.gg_collection_classify_files, handle, arr, nq, _dir_arg(cache_dir), rp, bp, bap)
        return best, best_ani

    def sketch_files(self, paths, cache_dir=None):
        """finch sketch_files (src/finch.rs:47) for files -> (sketches [n, s] u64
        padded with 0, lens [n] u32, number of genomes served by cache_dir)."""
        arr, n = _paths_arg(paths)
        op, lp, out, lens = _rows_out(n, self.s)
        hits = _u32()
        self._call(_L.gg_sketch_files, arr, n, _dir_arg(cache_dir), op, lp, _byref(hits))
        return out, lens, hits.value

    def sketch_files_stats(self, paths, cache_dir=None):
        """sketch_files plus every genome's GenomeAssemblyStats from the same
        read of each file (gg_sketch_files_stats) -> (sketches, lens, stats).
        cache_dir is written, never read: a later precluster_files over the
        same files, in any order, finds every sketch there."""
        arr, n = _paths_arg(paths)
        op, lp, out, lens = _rows_out(n, self.s)
        stats = np.zeros(max(n, 1), dtype=STATS_DTYPE)
        self._call(_L.gg_sketch_files_stats, arr, n, _dir_arg(cache_dir), op, lp, _ptr(stats))
        return out, lens, _stats_list(stats[:n])

    def precluster_files(self, paths, min_ani, cache_dir=None):
        """-> (pairs structured array sorted by (i, j), ani f32 array).  With
        cache_dir, genomes sketched by an earlier call are read from the
        sketch cache (self.last_cached counts them)."""
        arr, n = _paths_arg(paths)
        out, hits = _PairsOut(), _u32()
        st = _L.gg_precluster_files_cached(self._c, arr, n, _f32(min_ani), _dir_arg(cache_dir), *out.refs, _byref(hits))
        self.last_cached = hits.value  # (written on failure too, before the status is looked at)
        if st != GG_OK:
            raise self._err(st)
        return out.take()

    def precluster_files_resident(self, paths, min_ani, cache_dir=None):
        """precluster_files with the rows resident on the (first) device
        (gg_precluster_files_resident): the pairs by the context's pairs path
        (set_pairs_path), sorted and given their f32 ANI on the device ->
        (pairs, ani, summary dict of gg_pairs_matrix_summary).  pairs and ani
        equal precluster_files' whatever the path."""
        arr, n = _paths_arg(paths)
        out, summary = _PairsOut(), _PairsMatrixSummary()
        self._call(_L.gg_precluster_files_resident, arr, n, _f32(min_ani), _dir_arg(cache_dir), *out.refs,
                   _byref(summary))
        pairs, ani = out.take()
        return pairs, ani, summary.as_dict()

    def pairs_matrix(self, sketches, lens, min_ani, rows=None):
        """pairs() over the listed rows (None: all of them) by the matrix
        product with the thresholded epilogue (gg_pairs_matrix, DESIGN.md
        4.12): for dense sets, where the inverted index pays g^2 reads per
        hash shared by g rows -> (pairs sorted by (i, j), summary dict of
        gg_pairs_matrix_summary).  rows may not repeat an index."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        if rows is None:
            r, rp, m = None, None, n
        else:  # (not _matrix_rows_arg: rows is not flattened here, a 2-D rows counts its first axis)
            r = np.ascontiguousarray(rows, dtype=np.uint32)
            rp, m = _ptr(r), len(r)
        out, summary = _PairsOut(ani=False), _PairsMatrixSummary()
        self._call(_L.gg_pairs_matrix, _ptr(sk), _ptr(ln), n, rp, m, _f32(min_ani), *out.refs, _byref(summary))
        return out.take(), summary.as_dict()

    def pairs_border_matrix(self, sketches, lens, n_old, min_ani):
        """pairs_border() by the border form of the matrix product
        (gg_pairs_border_matrix): for new strains added to a
        dense set -> (pairs sorted by (i, j), summary dict of
        gg_pairs_matrix_summary; its column counts are the border's)."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        out, summary = _PairsOut(ani=False), _PairsMatrixSummary()
        self._call(_L.gg_pairs_border_matrix, _ptr(sk), _ptr(ln), n, int(n_old), _f32(min_ani), *out.refs,
                   _byref(summary))
        return out.take(), summary.as_dict()

    def set_pairs_path(self, path):
        """What produces the pairs inside cluster_rows_device,
        cluster_files_resident, precluster_matrices_files,
        precluster_files_resident and the border calls pairs_border,
        pairs_border_device and update_files: "default" (K2), "matrix" (the
        pair form of the matrix product, for a border its border form) or
        "auto" (the product when the index is certainly the dearer,
        gg_set_pairs_path) -> the path that was set before."""
        if path not in PAIRS_PATHS:
            raise ValueError("pairs path must be one of %s, not %r" % (", ".join(PAIRS_PATHS), path))
        before = self.pairs_path
        self._call(_L.gg_set_pairs_path, PAIRS_PATHS.index(path))
        return before

    @property
    def pairs_path(self):
        return PAIRS_PATHS[_L.gg_pairs_path(self._c)]

    def pairs_paths_taken(self):
        """Calls that needed pairs of resident rows since creation, by what
        ran: {"default", "matrix", "auto"} (auto: the matrix by AUTO's choice)."""
        return {k: int(v) for k, v in zip(PAIRS_PATHS, self._counters(_L.gg_pairs_paths_taken, 3))}

    def cluster_pairs(self, n_genomes, pairs, ani, cluster_ani):
        """cluster_pairs_host on the context's (first) device -> rep_of."""
        p, a = _pairs_ani_arg(pairs, ani)
        rep_of = np.zeros(max(n_genomes, 1), np.uint32)
        self._call(_L.gg_cluster_pairs, n_genomes, _ptr(p), _ptr(a), len(p), _f32(cluster_ani), _ptr(rep_of))
        return rep_of[:n_genomes]

    def preclusters(self, n_genomes, pairs, with_pairs=True):
        """partition_preclusters + precluster_pairs as one call on the
        context's (first) device -> (members, offsets, local, pair_offsets),
        the same arrays as the two host functions give (duplicates of one pair
        in ascending src); local and pair_offsets are None without with_pairs."""
        p = _as_pairs(pairs)
        members = np.zeros(max(n_genomes, 1), np.uint32)
        offsets = np.zeros(n_genomes + 1, np.uint32)
        local = np.zeros(max(len(p), 1), LOCAL_PAIR_DTYPE) if with_pairs else None
        poff = np.zeros(n_genomes + 1, np.uint64) if with_pairs else None
        ns = _u32()
        self._call(_L.gg_preclusters, n_genomes, _ptr(p), len(p), _ptr(members), _ptr(offsets), _byref(ns),
                   _ptr(local) if with_pairs else None, _ptr(poff) if with_pairs else None)
        members, offsets = members[:n_genomes], offsets[:ns.value + 1].copy()
        if not with_pairs:
            return members, offsets, None, None
        return members, offsets, local[:len(p)], poff[:ns.value + 1].copy()

    def ani_pairs(self, sketches, lens, pairs):
        """ani_pairs_host on the context's (first) device, one kernel launch
        for the whole list -> (PAIR_DTYPE array in the order given, ani f32)."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        p = _pair_list_arg(pairs)
        ani = np.zeros(max(len(p), 1), np.float32)
        self._call(_L.gg_ani_pairs, _ptr(sk), _ptr(ln), n, _ptr(p), len(p), _ptr(ani))
        return p, ani[:len(p)]

    def ani_matrix(self, sketches, lens, rows=None):
        """ani_matrix_host on the context's (first) device: the shared-hash
        counts as one product on the matrix cores ->
        (common, total, ani, summary dict of gg_matrix_summary)."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        r, rp, m = _matrix_rows_arg(rows, n)
        common, total, ani = _matrix_out(m)
        summary = _MatrixSummary()
        self._call(_L.gg_ani_matrix, _ptr(sk), _ptr(ln), n, rp, m, _ptr(common), _ptr(total), _ptr(ani),
                   _byref(summary))
        return common[:m, :m], total[:m, :m], ani[:m, :m], summary.as_dict()

    def ani_matrix_files(self, paths, cache_dir=None):
        """sketch_files(paths, cache_dir) followed by ani_matrix over all rows
        (gg_ani_matrix_files) -> (common, total, ani, summary dict)."""
        arr, m = _paths_arg(paths)
        common, total, ani = _matrix_out(m)
        summary = _MatrixSummary()
        # (not _dir_arg: "" is NULL in this call and in precluster_matrices_files)
        self._call(_L.gg_ani_matrix_files, arr, m, os.fsencode(cache_dir) if cache_dir else None, _ptr(common),
                   _ptr(total), _ptr(ani), _byref(summary))
        return common[:m, :m], total[:m, :m], ani[:m, :m], summary.as_dict()

    def ani_matrix_groups(self, sketches, lens, members, offsets=None):
        """ani_matrix_groups_host on the context's (first) device: the
        matrix of every group in one call, the product seeing one group's
        columns at a time -> (common, total, ani,
        cell_offsets, summary dict).  No cap on the number of rows.  The
        call sorts every sketch entry once, about 1.6 ms per 10^7 sketch
        slots whatever the groups are: for groups below about 60 rows (at
        sketch size 1000) naming the pairs -- ani_pairs_device +
        ani_f32_device -- reaches the same cells faster (0.36 against
        1.64 ms on 10,000 rows in groups of 10); above it this call wins."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        mem, off, ng, cells, common, total, ani = _groups_out(members, offsets)
        summary = _MatrixSummary()
        self._call(_L.gg_ani_matrix_groups, _ptr(sk), _ptr(ln), n, _ptr(mem), _ptr(off), ng, _ptr(common), _ptr(total),
                   _ptr(ani), _byref(summary))
        z = int(cells[-1])
        return common[:z], total[:z], ani[:z], cells, summary.as_dict()

    def precluster_matrices_files(self, paths, min_ani, cache_dir=None):
        """The ANI matrix of every precluster of the files
        (gg_precluster_matrices_files): sketches as precluster_files, then K2
        at min_ani, the partition and the grouped matrices on the resident
        rows -> (members, offsets, cell_offsets, common, total, ani, summary
        dict); the groups are preclusters()' (largest first)."""
        arr, n = _paths_arg(paths)
        mem, off, cel, com, tot, an = _vp(), _vp(), _vp(), _vp(), _vp(), _vp()
        ng = _u32()
        summary = _MatrixSummary()
        # (not _dir_arg: "" is NULL in this call and in ani_matrix_files)
        self._call(_L.gg_precluster_matrices_files, arr, n, _f32(min_ani), os.fsencode(cache_dir) if cache_dir else None,
                   _byref(mem), _byref(off), _byref(ng), _byref(cel), _byref(com), _byref(tot), _byref(an),
                   _byref(summary))
        offsets = _take_array(off, ng.value + 1, np.uint32)
        cells = _take_array(cel, ng.value + 1, np.uint64)
        # (members is allocated for one entry at least; every buffer is released)
        members = _take_array(mem, n, np.uint32)
        z = int(cells[-1])
        return (members, offsets, cells, _take_array(com, z, np.uint32), _take_array(tot, z, np.uint32),
                _take_array(an, z, np.float32), summary.as_dict())

    def validate_clusters(self, sketches, lens, clusters, ani):
        """validate_clusters_host on the device (gg_validate_clusters): the
        members through the named-pair kernel, the representatives through
        the all-pairs path -> Validation."""
        sk, ln, n, _ = _rows_arg(sketches, lens, self.s)
        members, offsets, nc = _clusters_arg(clusters)
        summary, bad = _Validation(), _PairsOut()
        self._call(_L.gg_validate_clusters, _ptr(sk), _ptr(ln), n, _ptr(members), _ptr(offsets), nc, _f32(ani),
                   _byref(summary), *bad.refs)
        return Validation(summary, *bad.take())

    def validate_files(self, paths, clusters, ani, cache_dir=None):
        """sketch_files(paths, cache_dir) followed by validate_clusters in one
        call (gg_validate_files): clusters index paths -> Validation."""
        arr, n = _paths_arg(paths)
        members, offsets, nc = _clusters_arg(clusters)
        summary, bad = _Validation(), _PairsOut()
        self._call(_L.gg_validate_files, arr, n, _ptr(members), _ptr(offsets), nc, _f32(ani), _dir_arg(cache_dir),
                   _byref(summary), *bad.refs)
        return Validation(summary, *bad.take())

    def cluster_files(self, paths, min_ani, cluster_ani, cache_dir=None, want_pairs=True):
        """precluster_files(min_ani) followed by cluster_pairs(cluster_ani)
        in one call -> (rep_of, pairs, ani), or rep_of alone with
        want_pairs=False (the library then frees the pairs)."""
        arr, n = _paths_arg(paths)
        rep_of = np.zeros(max(n, 1), np.uint32)
        out = _PairsOut()
        self._call(_L.gg_cluster_files, arr, n, _f32(min_ani), _f32(cluster_ani), _dir_arg(cache_dir), _ptr(rep_of),
                   *(out.refs if want_pairs else (None, None, None)))
        if not want_pairs:
            return rep_of[:n]
        pairs, ani = out.take()
        return rep_of[:n], pairs, ani

    def cluster_files_resident(self, paths, min_ani, cluster_ani, cache_dir=None):
        """cluster_files(..., want_pairs=False) with the pair list staying in
        device memory (gg_cluster_files_resident) -> (rep_of, summary): summary
        a dict of n_pairs, ani_rechecked, n_preclusters, largest_precluster and
        pair_passes.  A multi-device context takes cluster_files' path and
        reports ani_rechecked and pair_passes as 0; the rest is the same."""
        arr, n = _paths_arg(paths)
        rep_of = np.zeros(max(n, 1), np.uint32)
        summary = _ClusterSummary()
        self._call(_L.gg_cluster_files_resident, arr, n, _f32(min_ani), _f32(cluster_ani), _dir_arg(cache_dir),
                   _ptr(rep_of), _byref(summary))
        return rep_of[:n], summary.as_dict()

    def precluster_files_each(self, paths, min_ani, each, cache_dir=None):
        """precluster_files, and every compared pair (i < j, all N (N - 1) / 2,
        whatever the ANI) handed to each(block) in (i, j) order as PAIR_DTYPE
        arrays of at most ~4M pairs (gg_precluster_files_each: galah's debug
        level, src/finch.rs:65-68, without holding every pair).  each returning
        True stops the call (GalahGpuError, status 9)."""
        arr, n = _paths_arg(paths)
        out, hits = _PairsOut(), _u32()
        raised = []

        def sink(_user, ptr, n):
            try:
                blk = np.empty(n, dtype=PAIR_DTYPE)
                if n:
                    ctypes.memmove(blk.ctypes.data, ptr, n * PAIR_DTYPE.itemsize)
                return 1 if each(blk) else 0
            except BaseException as e:  # (an exception may not cross the C frame)
                raised.append(e)
                return 1

        cb = PAIR_SINK(sink)
        st = _L.gg_precluster_files_each(self._c, arr, n, _f32(min_ani), _dir_arg(cache_dir), cb, None, *out.refs,
                                         _byref(hits))
        self.last_cached = hits.value  # (as precluster_files; then the callback's exception, then the status)
        if raised:
            raise raised[0]
        if st != GG_OK:
            raise self._err(st)
        return out.take()

    # -- device-resident API (torch tensors on this context's device) ---------
    def sketch_device(self, d_words, runs, n_genomes, d_out, d_lens, stream=None):
        rp, nr, runs = _runs_arg(runs)
        self._call(_L.gg_sketch_device, _dev_ptr(d_words), d_words.numel(), rp, nr, n_genomes, _dev_ptr(d_out),
                   _dev_ptr(d_lens), stream)

    def pairs_device(self, d_sketches, d_lens, n, tile_begin, tile_end, min_ani, d_out, out_cap, d_count,
                     stream=None):
        self._call(_L.gg_pairs_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, tile_begin, tile_end, _f32(min_ani),
                   _dev_ptr(d_out), out_cap, _dev_ptr(d_count), stream)

    def pairs_border_device(self, d_sketches, d_lens, n, n_old, min_ani, d_out, out_cap, d_count, stream=None):
        """pairs_border over device-resident tensors, the contract of
        pairs_device (appends unsorted to d_out, d_count incremented by the
        number found, entries past out_cap dropped; asynchronous).  d_sketches
        may be a tensor with spare rows kept between updates: a batch of new
        sketches is written after the n_old rows it holds and only n grows."""
        self._call(_L.gg_pairs_border_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, int(n_old), _f32(min_ani),
                   _dev_ptr(d_out), out_cap, _dev_ptr(d_count), stream)

    def cluster_pairs_device(self, n_genomes, d_pairs, d_ani, n_pairs, cluster_ani, d_rep_of, stream=None):
        """cluster_pairs over device-resident tensors: d_pairs n_pairs 16-byte
        gg_pair records, d_ani f32, d_rep_of u32 [n_genomes] (every entry is
        written).  Synchronises the stream; the input is not checked."""
        self._call(_L.gg_cluster_pairs_device, n_genomes, _dev_ptr(d_pairs), _dev_ptr(d_ani), n_pairs, _f32(cluster_ani),
                   _dev_ptr(d_rep_of), stream)

    def ani_f32_device(self, d_pairs, n_pairs, d_ani, d_ani_f64=None, stream=None):
        """d_ani[p] = ani_f32(common, total, k) of the n_pairs 16-byte gg_pair
        records at d_pairs, bit for bit, computed on the device; d_ani_f64
        (optional) the f64 before rounding -> the number of entries the host
        recomputed.  Synchronises the stream."""
        cnt = _u64()
        self._call(_L.gg_ani_f32_device, _dev_ptr(d_pairs), n_pairs, _dev_ptr(d_ani), _dev_opt(d_ani_f64), _byref(cnt),
                   stream)
        return cnt.value

    def cluster_rows_device(self, d_sketches, d_lens, n, min_ani, cluster_ani, d_rep_of, want_summary=True,
                            stream=None):
        """pairs + ani_f32 + cluster_pairs over device-resident rows, the pair
        list never leaving device memory: d_sketches [n, s] u64, d_lens [n]
        u32, d_rep_of u32 [n] (every entry is written) -> (summary, d_pairs,
        d_ani, n_pairs): summary as cluster_files_resident gives it (None
        without want_summary), d_pairs and d_ani the device addresses (ints) of
        the context's n_pairs unsorted gg_pair records and their f32 ANI, valid
        until the next call on the context.  Without want_summary the
        partition into preclusters is not computed and n_pairs is None.
        Synchronises the stream."""
        summary = _ClusterSummary()
        pp, ap = _vp(), _vp()
        self._call(_L.gg_cluster_rows_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, _f32(min_ani),
                   _f32(cluster_ani), _dev_ptr(d_rep_of), _byref(summary) if want_summary else None, _byref(pp),
                   _byref(ap), stream)
        if not want_summary:
            return None, pp.value or 0, ap.value or 0, None
        return summary.as_dict(), pp.value or 0, ap.value or 0, int(summary.n_pairs)

    def preclusters_device(self, n_genomes, d_pairs, n_pairs, d_members, d_offsets, d_local=None,
                           d_pair_offsets=None, stream=None):
        """preclusters over device-resident tensors (or pointers): d_pairs
        n_pairs 16-byte gg_pair records, d_members u32 [n_genomes], d_offsets
        u32 [n_genomes + 1], d_local n_pairs 16-byte gg_local_pair records,
        d_pair_offsets u64 [n_genomes + 1] (both None: the partition only)
        -> n_sets.  Synchronises the stream; the input is not checked: a pair
        with an index >= n_genomes is left out, and d_pair_offsets[n_sets] is
        the number of local pairs written."""
        ns = _u32()
        self._call(_L.gg_preclusters_device, n_genomes, _dev_ptr(d_pairs), n_pairs, _dev_ptr(d_members),
                   _dev_ptr(d_offsets), _byref(ns), _dev_opt(d_local), _dev_opt(d_pair_offsets), stream)
        return ns.value

    def ani_pairs_device(self, d_sketches, d_lens, n, d_list, m, stream=None):
        """ani_pairs over device-resident tensors: d_sketches [n, s] u64,
        d_lens [n] u32, d_list m 16-byte gg_pair records whose common and total
        are written in place (the integers only; ani_f32 gives the value).
        Asynchronous; the input is not checked: an entry with an index >= n
        receives 0 and 0."""
        self._call(_L.gg_ani_pairs_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, _dev_ptr(d_list), m, stream)

    def pairs_matrix_device(self, d_sketches, d_lens, n, d_rows, m, min_ani, d_out, out_cap, d_count,
                            want_summary=True, stream=None):
        """pairs_matrix over device-resident tensors, the output contract of
        pairs_device: the passing pairs among the m listed rows (d_rows None:
        rows 0 .. m-1) appended unsorted to d_out, d_count (u64) grown by the
        number found, nothing written past out_cap.  d_rows is not checked: an
        index >= n is an empty row, a row listed twice gets its pairs once per
        position.  Synchronises the stream -> summary dict (None without
        want_summary; n_pairs may exceed out_cap)."""
        summary = _PairsMatrixSummary()
        self._call(_L.gg_pairs_matrix_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, _dev_opt(d_rows), m,
                   _f32(min_ani), _dev_ptr(d_out), out_cap, _dev_ptr(d_count),
                   _byref(summary) if want_summary else None, stream)
        return summary.as_dict() if want_summary else None

    def pairs_border_matrix_device(self, d_sketches, d_lens, n, n_old, min_ani, d_out, out_cap, d_count,
                                   want_summary=True, stream=None):
        """pairs_border_matrix over device-resident tensors, the output
        contract of pairs_border_device: the border's passing pairs appended
        unsorted to d_out, d_count (u64) grown by the number found, nothing
        written past out_cap; n_old == n runs nothing.  Synchronises the
        stream -> summary dict (None without want_summary; n_pairs may exceed
        out_cap)."""
        summary = _PairsMatrixSummary()
        self._call(_L.gg_pairs_border_matrix_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, int(n_old),
                   _f32(min_ani), _dev_ptr(d_out), out_cap, _dev_ptr(d_count),
                   _byref(summary) if want_summary else None, stream)
        return summary.as_dict() if want_summary else None

    def ani_matrix_device(self, d_sketches, d_lens, n, d_rows, m, d_common=None, d_total=None, d_ani=None,
                          stream=None):
        """ani_matrix over device-resident tensors: d_sketches [n, s] u64,
        d_lens [n] u32 (as i32 tensors), d_rows [m] row indices or None
        (positions are rows 0 .. m-1); d_common / d_total (i32) / d_ani (f32),
        each [m, m] or None, are written.  An index >= n is an empty row.
        Synchronises the stream -> summary dict."""
        summary = _MatrixSummary()
        self._call(_L.gg_ani_matrix_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, _dev_opt(d_rows), m,
                   _dev_opt(d_common), _dev_opt(d_total), _dev_opt(d_ani), _byref(summary), stream)
        return summary.as_dict()

    def ani_matrix_groups_device(self, d_sketches, d_lens, n, d_members, offsets, d_common=None, d_total=None,
                                 d_ani=None, stream=None):
        """ani_matrix_groups over device-resident tensors: d_members [P] row
        indices (i32 tensor), offsets a host array [n_groups + 1]; d_common /
        d_total (i32) / d_ani (f32), flat with ani_matrix_group_cells(offsets)[-1]
        entries or None, are written.  An index >= n is an empty row.
        Synchronises the stream -> summary dict."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        summary = _MatrixSummary()
        self._call(_L.gg_ani_matrix_groups_device, _dev_ptr(d_sketches), _dev_ptr(d_lens), n, _dev_opt(d_members),
                   _ptr(off), len(off) - 1, _dev_opt(d_common), _dev_opt(d_total), _dev_opt(d_ani), _byref(summary),
                   stream)
        return summary.as_dict()

    def synth_mixed_device(self, lens, cluster_size, max_sub_rate, n_run_rate, seed, d_words, stream=None,
                           first_genome=0):
        """Config C5: genomes of lengths `lens` (see synth_mixed_lengths) with
        N runs; -> the host run table (RUN_DTYPE)."""
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        cap = max(1024, int(lens.sum() * max(n_run_rate, 1e-6) * 2) + 4 * len(lens))
        for _ in range(2):
            runs = np.zeros(cap, dtype=RUN_DTYPE)
            nr = _u64()
            st = _L.gg_synth_mixed_device(self._c, first_genome, len(lens), _ptr(lens), cluster_size,
                                          _f32(max_sub_rate), _f64(n_run_rate), seed, _dev_ptr(d_words), _ptr(runs), cap,
                                          _byref(nr), stream)
            if st == GG_OK:
                return runs[:nr.value]
            if st != 8:  # (8: the run table was too small, nr holds the count: once more with that)
                raise self._err(st)
            cap = nr.value
        raise self._err(st)

    def synth_device(self, n_genomes, genome_len, cluster_size, max_sub_rate, seed, d_words, stream=None,
                     first_genome=0):
        runs = np.zeros(n_genomes, dtype=RUN_DTYPE)
        self._call(_L.gg_synth_clustered_device, first_genome, n_genomes, genome_len, cluster_size, _f32(max_sub_rate),
                   seed, _dev_ptr(d_words), _ptr(runs), stream)
        return runs


# ---------------------------------------------------------------------------
# Reference-interface mirror
# ---------------------------------------------------------------------------
def _rust_f32_debug(x):
    """Rust `{:?}` of an f32: shortest round-trip decimal, always with a '.'."""
    s = np.format_float_positional(np.float32(x), unique=True, trim="-")
    if "." not in s and "inf" not in s and "nan" not in s:
        s += ".0"
    return s


class SortedPairGenomeDistanceCache:
    """src/sorted_pair_genome_distance_cache.rs:4-59: a map keyed by (min, max)."""

    def __init__(self):
        self.internal = {}

    @staticmethod
    def _key(ids):
        a, b = ids
        return (a, b) if a < b else (b, a)

    def insert(self, genome_ids, distance):
        self.internal[self._key(genome_ids)] = distance

    def get(self, genome_ids):
        """Option<&Option<f32>>: KeyError-free; returns the stored value or the
        sentinel `MISSING` when absent."""
        return self.internal.get(self._key(genome_ids), MISSING)

    def contains_key(self, genome_ids):
        return self._key(genome_ids) in self.internal

    def transform_ids(self, input_ids):
        """:47-58 -- subset with ids re-numbered by position in input_ids."""
        out = SortedPairGenomeDistanceCache()
        for i, g1 in enumerate(input_ids):
            for j in range(i + 1, len(input_ids)):
                v = self.get((g1, input_ids[j]))
                if v is not MISSING:
                    out.insert((i, j), v)
        return out

    def __len__(self):
        return len(self.internal)

    def __eq__(self, other):
        if not isinstance(other, SortedPairGenomeDistanceCache):
            return NotImplemented
        if self.internal.keys() != other.internal.keys():
            return False
        for k, v in self.internal.items():
            w = other.internal[k]
            if (v is None) != (w is None):
                return False
            if v is not None and np.float32(v) != np.float32(w):
                return False
        return True

    def __repr__(self):
        items = ", ".join(
            "(%d, %d): %s" % (k[0], k[1], "None" if v is None else "Some(%s)" % _rust_f32_debug(v))
            for k, v in sorted(self.internal.items()))
        return "SortedPairGenomeDistanceCache { internal: {%s} }" % items


MISSING = object()


def _cache_of(pairs, ani):
    """The passing pairs and their f32 ANI as the cache finch::distances returns."""
    cache = SortedPairGenomeDistanceCache()
    for p, a in zip(pairs, ani):
        cache.insert((int(p["i"]), int(p["j"])), np.float32(a))
    return cache


class PreclusterDistanceFinder:
    """src/lib.rs:23-27."""

    def distances(self, genome_fasta_paths):
        raise NotImplementedError

    def method_name(self):
        raise NotImplementedError


_CTX_CACHE = {}


def _context(k, s, seed=0):
    """Every visible GPU (or GALAHGPU_DEVICES), as FinchPreclusterer::distances
    uses them; host ingest threads from GALAHGPU_THREADS / the affinity mask."""
    key = (k, s, seed)
    c = _CTX_CACHE.get(key)
    if c is None:
        c = Context(k, s, seed, devices="all")
        _CTX_CACHE[key] = c
    return c


@contextlib.contextmanager
def _under_pairs_path(ctx, path):
    """The body under pairs path `path` on a one-device context; the cached
    context is shared, so what was set before is put back after it.  path
    None, or a multi-device context: the body as it is."""
    if path is None or ctx.device_count != 1:
        yield
        return
    before = ctx.set_pairs_path(path)
    try:
        yield
    finally:
        ctx.set_pairs_path(before)


@contextlib.contextmanager
def _failing_as(what):
    """A GalahGpuError of the body as the RuntimeError "<what>: <the error>" galah's flow reports."""
    try:
        yield
    except GalahGpuError as e:
        raise RuntimeError("%s: %s" % (what, e)) from e


def _sketching():
    return _failing_as("Failed to sketch genomes with finch")  # src/finch.rs:50


def _clustering():
    return _failing_as("Failed to cluster genomes")


def _finch_only(who, preclusterer, clusterer):
    """initialise() and the one combination that runs here: both methods "finch"."""
    clusterer.initialise()
    pre_name, clu_name = preclusterer.method_name(), clusterer.method_name()
    if not (pre_name == clu_name == "finch"):
        raise NotImplementedError("galah_amd.%s: only finch + finch runs here, not %s + %s" % (who, pre_name, clu_name))


def _check_state(state, preclusterer):
    """ValueError when the state was made with another k, sketch size, seed or min_ani."""
    mine = (preclusterer.kmer_length, preclusterer.num_kmers, 0, np.float32(preclusterer.min_ani).tobytes())
    if (state.k, state.s, state.seed, np.float32(state.min_ani).tobytes()) != mine:
        raise ValueError("PreclusterState of k=%d s=%d seed=%d min_ani=%r, preclusterer of k=%d s=%d seed=0 "
                         "min_ani=%r" % (state.k, state.s, state.seed, state.min_ani, preclusterer.kmer_length,
                                         preclusterer.num_kmers, preclusterer.min_ani))


def _new_paths(paths, present):
    """The paths as strings; ValueError on one already present or given twice."""
    new = [os.fspath(p) for p in paths]
    seen = set(present)
    for p in new:
        if p in seen:
            raise ValueError("genome already present: %s" % p)
        seen.add(p)
    return new


def distances(genome_fasta_paths, min_ani, num_kmers, kmer_length, sketch_cache_dir=None, pairs_path=None):
    """src/finch.rs:26-75 -> SortedPairGenomeDistanceCache, computed on the GPU.
    sketch_cache_dir (not in galah) reuses sketches of
    unchanged genome files from earlier runs; the result is the same.
    pairs_path ("default", "matrix" or "auto"; None: the call below as ever)
    takes Context.precluster_files_resident under that path on a one-device
    context.  It is ignored, the result being the same, at debug level (every
    compared pair must be logged: the streaming call stays) and on a
    multi-device context (the resident call is not sharded)."""
    log = logging.getLogger("galah")
    # At debug level the reference logs every compared pair
    # (src/finch.rs:65-68): the library then streams all N (N - 1) / 2 pairs
    # in row blocks (gg_precluster_files_each), each logged with its f64
    # distance in the reference's loop order; the cache is filled from the
    # passing pairs as at any other level, so no block outlives its lines.
    every = log.isEnabledFor(logging.DEBUG)
    paths = list(genome_fasta_paths)
    k = int(kmer_length)

    def each(block):
        for p in block:
            d = ani_f64(int(p["common"]), int(p["total"]), k)
            log.debug("Comparing %s and %s, distance %s", paths[int(p["i"])], paths[int(p["j"])], rust_f64(d))
        return False

    with _sketching():
        ctx = _context(k, int(num_kmers))
        log.info("Sketching MinHash representations of each genome with finch ..")  # src/finch.rs:46
        thr = float(np.float32(min_ani))
        if every:
            pairs, ani = ctx.precluster_files_each(paths, thr, each, cache_dir=sketch_cache_dir)
        elif pairs_path is not None and ctx.device_count == 1:
            with _under_pairs_path(ctx, pairs_path):
                pairs, ani, _ = ctx.precluster_files_resident(paths, thr, cache_dir=sketch_cache_dir)
        else:
            pairs, ani = ctx.precluster_files(paths, thr, cache_dir=sketch_cache_dir)
    log.info("Finished sketching genomes")  # src/finch.rs:48
    log.info(ctx.info_line())  # device count, phase times, fallbacks (gg_info_line)
    return _cache_of(pairs, ani)


def rust_f64(x):
    """Rust's `{}` of an f64: the shortest round-trip digits, no exponent, no
    trailing ".0" (1.0 -> "1", 0.0 -> "0")."""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    r = repr(x)
    if "e" in r or "E" in r:
        m, e = r.lower().split("e")
        neg = m.startswith("-")
        m = m.lstrip("-")
        digits = m.replace(".", "")
        point = (m.index(".") if "." in m else len(m)) + int(e)
        if point <= 0:
            r = "0." + "0" * (-point) + digits
        elif point >= len(digits):
            r = digits + "0" * (point - len(digits))
        else:
            r = digits[:point] + "." + digits[point:]
        r = ("-" if neg else "") + r
    if r.endswith(".0"):
        r = r[:-2]
    return r


class FinchPreclusterer(PreclusterDistanceFinder):
    """src/finch.rs:4-24: min_ani is a fraction (f32), num_kmers = s, kmer_length = k."""

    def __init__(self, min_ani, num_kmers=1000, kmer_length=21, sketch_cache_dir=None, pairs_path=None):
        """pairs_path: None (the default K2 through the calls used so far),
        or "default" / "matrix" / "auto": distances() and cluster() then run
        the resident calls under that pairs path (Context.set_pairs_path;
        "matrix" suits thousands of strains of one species), and update()
        (so distances_state() and cluster_update()) evaluates its border
        under it.  The results do
        not depend on it.  It is ignored on a multi-device context and, in
        distances(), at debug level (see distances).  The path is set on the
        shared cached context around the call and put back after it: two
        threads with different pairs paths can switch each other's route (and
        what pairs_paths_taken counts) mid-call, never a result."""
        if pairs_path is not None and pairs_path not in PAIRS_PATHS:
            raise ValueError("pairs_path must be None or one of %s, not %r" % (", ".join(PAIRS_PATHS), pairs_path))
        self.min_ani = np.float32(min_ani)
        self.num_kmers = int(num_kmers)
        self.kmer_length = int(kmer_length)
        self.sketch_cache_dir = sketch_cache_dir
        self.pairs_path = pairs_path

    def distances(self, genome_fasta_paths):
        if self.pairs_path is None:
            return distances(genome_fasta_paths, self.min_ani, self.num_kmers, self.kmer_length,
                             sketch_cache_dir=self.sketch_cache_dir)
        return distances(genome_fasta_paths, self.min_ani, self.num_kmers, self.kmer_length,
                         sketch_cache_dir=self.sketch_cache_dir, pairs_path=self.pairs_path)

    def method_name(self):
        return "finch"

    def distances_state(self, genome_fasta_paths):
        """distances() that can be carried forward: a PreclusterState of the
        paths, their sketches and the passing pairs (state.cache() is what
        distances() returns)."""
        empty = PreclusterState([], np.zeros((0, self.num_kmers), np.uint64), np.zeros(0, np.uint32),
                                np.zeros(0, PAIR_DTYPE), np.zeros(0, np.float32), self.kmer_length, self.num_kmers, 0,
                                self.min_ani)
        return self.update(empty, genome_fasta_paths)

    def collection(self, reserve=0):
        """An empty Collection (resident on the GPU) with this preclusterer's
        k, sketch size, min_ani, sketch cache directory and pairs path;
        reserve: genomes to make room for at once."""
        return Collection(self, reserve=reserve)

    def update(self, state, new_paths):
        """Adds genomes to a finished run -> a PreclusterState over state.paths
        + new_paths whose cache() equals distances(state.paths + new_paths):
        only the new files are read and sketched, and only the pairs that
        involve a new genome are evaluated (Context.update_files).  ValueError
        when the state was made with another k, sketch size, seed or min_ani,
        or when a new path is already present."""
        new_paths = [os.fspath(p) for p in new_paths]  # (first, as ever: a TypeError here comes before the state's ValueError)
        _check_state(state, self)
        new_paths = _new_paths(new_paths, state.paths)
        with _sketching():
            ctx = _context(self.kmer_length, self.num_kmers)
            with _under_pairs_path(ctx, self.pairs_path):
                sk, lens, border, border_ani = ctx.update_files(state.sketches, state.lens, new_paths,
                                                                float(self.min_ani), cache_dir=self.sketch_cache_dir)
        pairs = np.concatenate([state.pairs, border])
        ani = np.concatenate([state.ani, border_ani])
        by_ij = np.lexsort((pairs["j"], pairs["i"]))  # SortedPairGenomeDistanceCache order
        return PreclusterState(state.paths + new_paths, np.concatenate([state.sketches, sk]),
                               np.concatenate([state.lens, lens]), pairs[by_ij], ani[by_ij], state.k, state.s,
                               state.seed, state.min_ani)


class PreclusterState:
    """A finished precluster run that genomes can be added to: the paths, their
    sketches [n, s] u64 and lens [n] u32, the passing pairs (PAIR_DTYPE, sorted
    by (i, j)) with their f32 ANI, and the parameters they were made with (k,
    s, seed, min_ani).  FinchPreclusterer.distances_state makes one,
    FinchPreclusterer.update carries it forward."""

    def __init__(self, paths, sketches, lens, pairs, ani, k, s, seed, min_ani):
        self.paths = [os.fspath(p) for p in paths]
        self.sketches = np.ascontiguousarray(sketches, dtype=np.uint64).reshape(len(self.paths), int(s))
        self.lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(len(self.paths))
        self.pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE).reshape(-1)
        self.ani = np.ascontiguousarray(ani, dtype=np.float32).reshape(len(self.pairs))
        self.k, self.s, self.seed, self.min_ani = int(k), int(s), int(seed), np.float32(min_ani)

    def cache(self):
        """The pairs as FinchPreclusterer.distances returns them."""
        return _cache_of(self.pairs, self.ani)

    def save(self, file):
        """One .npz of plain arrays (no pickled objects): a path or a binary
        file object.  Paths are stored as their file-system bytes."""
        raw = [os.fsencode(p) for p in self.paths]
        ends = np.cumsum([len(b) for b in raw], dtype=np.uint64) if raw else np.zeros(0, np.uint64)
        quads = np.stack([self.pairs[f] for f in ("i", "j", "common", "total")], axis=1).astype(np.uint32)
        np.savez(file, path_bytes=np.frombuffer(b"".join(raw), dtype=np.uint8), path_ends=ends,
                 sketches=self.sketches, lens=self.lens, pairs=quads.reshape(-1, 4), ani=self.ani,
                 params=np.array([self.k, self.s, self.seed], dtype=np.uint64),
                 min_ani=np.array([self.min_ani], dtype=np.float32))

    @classmethod
    def load(cls, file):
        with np.load(file, allow_pickle=False) as z:
            blob, ends = z["path_bytes"].tobytes(), z["path_ends"].astype(np.int64)
            starts = np.concatenate([[0], ends[:-1]]) if len(ends) else ends
            paths = [os.fsdecode(blob[a:b]) for a, b in zip(starts, ends)]
            quads = z["pairs"].reshape(-1, 4)
            pairs = np.zeros(len(quads), dtype=PAIR_DTYPE)
            for x, f in enumerate(("i", "j", "common", "total")):
                pairs[f] = quads[:, x]
            k, s, seed = (int(v) for v in z["params"])
            return cls(paths, z["sketches"], z["lens"], pairs, z["ani"], k, s, seed, z["min_ani"][0])


def _permutation(order, n=None):
    """order as an int64 array; ValueError unless it is a permutation of 0 .. n-1 (n None: of its own length)."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    n = len(order) if n is None else n
    if len(order) != n or (n and (order.min() < 0 or order.max() >= n or len(np.unique(order)) != n)):
        raise ValueError("order must be a permutation of 0 .. %d" % (n - 1))
    return order


def relabel_pairs(pairs, order):
    """The pairs of genomes numbered 0 .. n-1 renumbered by position in
    `order` (a permutation: position -> genome); i and j keep their places in
    each record, so a record may come out with i > j (cluster_pairs takes
    either orientation)."""
    order = _permutation(order)
    n = len(order)
    pos = np.empty(n, dtype=np.uint32)
    pos[order] = np.arange(n, dtype=np.uint32)
    out = np.array(pairs, dtype=PAIR_DTYPE).reshape(-1)
    if len(out) and (int(out["i"].max()) >= n or int(out["j"].max()) >= n):
        raise ValueError("pair index out of range of order")
    out["i"], out["j"] = pos[out["i"]], pos[out["j"]]
    return out


def cluster_update(state, new_paths, preclusterer, clusterer, order=None):
    """Adds new_paths to a finished run and clusters the union -> (clusters,
    new_state): preclusterer.update(state, new_paths), then the union's pairs
    relabelled through `order` and clustered on the device as cluster() does.
    order is a permutation of the union, position -> index into state.paths +
    new_paths (galah clusters in the order it is given: quality order); the
    default is the old genomes in their order, then the new ones as given, so
    that old representatives keep precedence.  clusters are lists of positions
    in that order, each with its representative first: what
    cluster([paths[g] for g in order], ...) returns."""
    _finch_only("cluster_update", preclusterer, clusterer)
    new_state = preclusterer.update(state, new_paths)
    n = len(new_state.paths)
    pairs = relabel_pairs(new_state.pairs, np.arange(n) if order is None else order)
    with _clustering():
        rep_of = _context(preclusterer.kmer_length, preclusterer.num_kmers).cluster_pairs(
            n, pairs, new_state.ani, float(np.float32(clusterer.get_ani_threshold())))
    return clusters_from_reps(rep_of), new_state


class Collection:
    """A set of genomes kept on the GPU between calls (gg_collection_*,
    DESIGN.md 4.15): their sketches, the passing pairs at the preclusterer's
    min_ani and their f32 ANI stay in device memory; add() reads and sketches
    only the new files and evaluates only their border, remove() filters and
    renumbers, cluster() relabels into any order and clusters.  Every result
    equals what FinchPreclusterer.distances / cluster give from scratch on
    .paths.  A context manager; FinchPreclusterer.collection() makes one."""

    def __init__(self, preclusterer, reserve=0, _handle=None, _paths=()):
        self._pre = preclusterer
        self._ctx = _context(preclusterer.kmer_length, preclusterer.num_kmers)
        self._paths = list(_paths)
        self._h = None
        with _failing_as("Failed to make a collection"):
            self._h = _handle if _handle is not None else self._ctx.collection_create(
                float(np.float32(preclusterer.min_ani)), reserve_rows=reserve, reserve_pairs=0)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_c", None):  # (a handle outlives its context only at interpreter exit)
                self._ctx.collection_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return len(self._paths)

    @property
    def paths(self):
        return list(self._paths)

    def info(self):
        return self._ctx.collection_stat(self._h)[0]

    def add(self, paths):
        """Adds genomes (files) -> the number of pairs added.  ValueError on a
        path already present; a file that cannot be read or parsed leaves the
        collection as it was."""
        new = _new_paths(paths, self._paths)
        # (under the preclusterer's pairs path, as FinchPreclusterer.update routes its border)
        with _sketching(), _under_pairs_path(self._ctx, self._pre.pairs_path):
            added = self._ctx.collection_add_files(self._h, new, cache_dir=self._pre.sketch_cache_dir)
        self._paths += new
        return added

    def remove(self, paths):
        """Removes genomes by path (ValueError on one that is not present);
        the others keep their relative order."""
        index = {p: x for x, p in enumerate(self._paths)}
        rows = []
        for p in paths:
            p = os.fspath(p)
            if p not in index:
                raise ValueError("genome not present: %s" % p)
            rows.append(index[p])
        new_index = self._ctx.collection_remove(self._h, rows)
        self._paths = [p for x, p in enumerate(self._paths) if new_index[x] != 0xFFFFFFFF]

    def cache(self):
        """The pairs as FinchPreclusterer.distances(self.paths) returns them."""
        return _cache_of(*self._ctx.collection_pairs(self._h))

    def cluster(self, clusterer, order=None):
        """The clusters of the collection's genomes as cluster_update returns
        them: lists of positions in `order` (position -> index into .paths;
        None: the paths' order), each with its representative first."""
        _finch_only("Collection.cluster", self._pre, clusterer)
        if order is not None:
            order = _permutation(order, len(self._paths))
        with _clustering():
            rep_of = self._ctx.collection_cluster(self._h, float(np.float32(clusterer.get_ani_threshold())), order)
        return clusters_from_reps(rep_of)

    def query(self, paths, min_ani=None):
        """The genomes of the collection each file is close to, without adding
        it: per path a list of (index into .paths, np.float32 ani), ANI
        descending, then index.  min_ani (a fraction): None, the
        preclusterer's.  A path already in the collection is allowed (it finds
        itself at ANI 1.0).  The collection is not changed."""
        qp = [os.fspath(p) for p in paths]
        thr = float(np.float32(self._pre.min_ani if min_ani is None else min_ani))
        with _sketching():
            pairs, ani = self._ctx.collection_query_files(self._h, qp, thr, cache_dir=self._pre.sketch_cache_dir)
        n = len(self._paths)
        out = [[] for _ in qp]
        for p, a in zip(pairs, ani):
            out[int(p["j"]) - n].append((int(p["i"]), np.float32(a)))
        for hits in out:
            hits.sort(key=lambda h: (-float(h[1]), h[0]))
        return out

    def classify(self, paths, clusterer, order=None):
        """What galah would decide for each file appended last to the
        clustering of the collection in `order` (as cluster takes it), each
        decided alone: None when the genome would be a new representative,
        else (index into .paths of its representative, np.float32 ani).  The
        collection is not changed."""
        _finch_only("Collection.classify", self._pre, clusterer)
        n = len(self._paths)
        if order is not None:
            order = _permutation(order, n)
        threshold = np.float32(clusterer.get_ani_threshold())
        qp = [os.fspath(p) for p in paths]
        with _clustering():
            rep_of = self._ctx.collection_cluster(self._h, float(threshold), order)
        # rank[row] = the representative's position in the order; other rows are no candidates
        rows = np.arange(n, dtype=np.int64) if order is None else order
        rank = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        reps = np.nonzero(rep_of == np.arange(n, dtype=np.uint32))[0]
        rank[rows[reps]] = reps.astype(np.uint32)
        with _sketching():
            best, best_ani = self._ctx.collection_classify_files(self._h, qp, rank,
                                                                 cache_dir=self._pre.sketch_cache_dir)
        return [None if int(b["i"]) == 0xFFFFFFFF or not np.float32(a) >= threshold else (int(b["i"]), np.float32(a))
                for b, a in zip(best, best_ani)]

    def state(self):
        """A PreclusterState of the collection (save / load as ever)."""
        sk, lens = self._ctx.collection_rows(self._h)
        pairs, ani = self._ctx.collection_pairs(self._h)
        return PreclusterState(self._paths, sk, lens, pairs, ani, self._pre.kmer_length, self._pre.num_kmers, 0,
                               self._pre.min_ani)

    @classmethod
    def from_state(cls, state, preclusterer):
        """A collection holding a PreclusterState (gg_collection_load: the
        pairs are checked for form and trusted, not recomputed).  ValueError
        when the state was made with another k, sketch size, seed or min_ani."""
        _check_state(state, preclusterer)
        ctx = _context(preclusterer.kmer_length, preclusterer.num_kmers)
        try:
            h = ctx.collection_load(state.sketches, state.lens, state.pairs, state.ani,
                                    float(np.float32(preclusterer.min_ani)))
        except GalahGpuError as e:
            raise ValueError("not a saved collection state: %s" % e) from e
        return cls(preclusterer, _handle=h, _paths=state.paths)


class ClusterDistanceFinder:
    """src/lib.rs:29-37."""

    def initialise(self):
        raise NotImplementedError

    def method_name(self):
        raise NotImplementedError

    def get_ani_threshold(self):
        raise NotImplementedError

    def calculate_ani(self, fasta1, fasta2):
        raise NotImplementedError


class FinchClusterer(ClusterDistanceFinder):
    """A finch clusterer: the ClusterDistanceFinder whose value for a pair is
    the one FinchPreclusterer stores (the original design of
    src/clusterer.rs, find_minhash_representatives / find_minhash_memberships;
    galah's CLUSTER_METHODS has no finch).  ani is a fraction (f32)."""

    def __init__(self, ani, num_kmers=1000, kmer_length=21):
        self.ani = np.float32(ani)
        self.num_kmers = int(num_kmers)
        self.kmer_length = int(kmer_length)

    def initialise(self):
        pass

    def method_name(self):
        return "finch"

    def get_ani_threshold(self):
        return self.ani

    def calculate_ani(self, fasta1, fasta2):
        """Option<f32>: the two files through precluster_files at min_ani 0."""
        _, ani = _context(self.kmer_length, self.num_kmers).precluster_files([fasta1, fasta2], 0.0)
        return np.float32(ani[0]) if len(ani) else None

    def calculate_ani_many(self, pairs_of_paths, sketch_cache_dir=None):
        """calculate_ani for a list of (fasta1, fasta2): every distinct file
        sketched once (from sketch_cache_dir when it has it), then one
        named-pair call -> a list of f32, in the order given."""
        index, paths, named = {}, [], []
        for a, b in pairs_of_paths:
            for p in (a, b):
                if p not in index:
                    index[p] = len(paths)
                    paths.append(p)
            named.append((index[a], index[b]))
        if not named:
            return []
        ctx = _context(self.kmer_length, self.num_kmers)
        sk, lens, _ = ctx.sketch_files(paths, cache_dir=sketch_cache_dir)
        _, ani = ctx.ani_pairs(sk, lens, named)
        return [np.float32(a) for a in ani]


def cluster(genomes, preclusterer, clusterer, sketch_cache_dir=None):
    """src/clusterer.rs:14-125 -> the clusters as lists of genome indices,
    each with its representative first.  Built for the case the reference
    marks skip_clusterer (:29-33): preclusterer and clusterer both "finch",
    the result then being a function of the pair cache, computed on the GPU
    (gg_cluster_files_resident on one device, the pairs never leaving it;
    gg_cluster_files on several).  Any other combination raises: the external-clusterer
    flow is not part of this library."""
    log = logging.getLogger("galah")
    clusterer.initialise()
    pre_name, clu_name = preclusterer.method_name(), clusterer.method_name()
    log.info("Preclustering with %s and clustering with %s", pre_name, clu_name)  # :24-27
    if not (pre_name == clu_name == "finch"):
        raise NotImplementedError("galah_amd.cluster: only finch + finch (the clusterer reusing the preclusterer's "
                                  "ANI values) runs here, not %s + %s" % (pre_name, clu_name))
    log.info("Preclustering and clustering methods are the same, so reusing ANI values")  # :31
    paths = list(genomes)
    cache_dir = sketch_cache_dir if sketch_cache_dir is not None else getattr(preclusterer, "sketch_cache_dir", None)
    with _sketching():
        ctx = _context(preclusterer.kmer_length, preclusterer.num_kmers)
        log.info("Sketching MinHash representations of each genome with finch ..")  # src/finch.rs:46
        min_ani, T = float(np.float32(preclusterer.min_ani)), float(np.float32(clusterer.get_ani_threshold()))
        if ctx.device_count == 1:
            # one device: the pair list stays in its memory, the preclusters'
            # count and largest size come back with rep_of
            with _under_pairs_path(ctx, getattr(preclusterer, "pairs_path", None)):
                rep_of, summary = ctx.cluster_files_resident(paths, min_ani, T, cache_dir=cache_dir)
            n_sets, largest = summary["n_preclusters"], summary["largest_precluster"]
        else:
            rep_of, pairs, _ = ctx.cluster_files(paths, min_ani, T, cache_dir=cache_dir)
            if paths:
                _, offsets = partition_preclusters(len(paths), pairs)
                n_sets, largest = len(offsets) - 1, int(offsets[1] - offsets[0])
    log.info("Finished sketching genomes")  # src/finch.rs:48
    log.info(ctx.info_line())
    log.info("Preclustering ..")  # :38
    if paths:
        log.info("Found %d preclusters. The largest contained %d genomes", n_sets, largest)  # :59-63
    log.info("Finding representative genomes and assigning all genomes to these ..")  # :65
    return clusters_from_reps(rep_of)


def rust_f32(x):
    """Rust's `{}` of an f32: the shortest round-trip digits, no exponent, no
    trailing ".0"."""
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def ani_matrix(genomes, num_kmers=1000, kmer_length=21, sketch_cache_dir=None):
    """The finch ANI between every two of the genomes (paths): each file
    sketched once (from sketch_cache_dir when it has it), then one dense
    matrix call on the GPU -> an [N, N] float32 array, symmetric, the value
    galah stores for each pair (1.0 on the diagonal of a non-empty genome)."""
    genomes = list(genomes)
    if not genomes:
        return np.zeros((0, 0), np.float32)
    ctx = _context(kmer_length, num_kmers)
    _, _, ani, _ = ctx.ani_matrix_files(genomes, cache_dir=sketch_cache_dir)
    return ani


def precluster_ani_matrices(genomes, precluster_ani=0.9, num_kmers=1000, kmer_length=21, sketch_cache_dir=None):
    """The finch ANI table of every precluster of the genomes (paths): the
    files sketched once, the preclusters at precluster_ani (a fraction, or a
    percentage as parse_percentage reads it) and each one's dense matrix in
    one grouped call on the GPU -> a list of (indices into genomes, [m, m]
    float32 block), largest precluster first; write_ani_matrix writes a block.
    (Where every precluster is smaller than about 60 genomes the named-pair
    path is the faster way to the same values, Context.ani_matrix_groups.)"""
    genomes = list(genomes)
    if not genomes:
        return []
    ctx = _context(kmer_length, num_kmers)
    members, offsets, cells, _, _, ani, _ = ctx.precluster_matrices_files(genomes, parse_percentage(precluster_ani),
                                                                          cache_dir=sketch_cache_dir)
    return [(members[offsets[g]:offsets[g + 1]].tolist(), ani_matrix_block(ani, offsets, cells, g))
            for g in range(len(offsets) - 1)]


def write_ani_matrix(f, genomes, ani):
    """The matrix as a TSV: a header row of the genomes' names (after an
    empty corner cell), then one row per genome, its name and its values as
    Rust prints an f32 (rust_f32).  f: a file object (text or binary) or a
    path."""
    ani = np.asarray(ani, dtype=np.float32)
    if ani.shape != (len(genomes), len(genomes)):
        raise ValueError("ani must be [len(genomes), len(genomes)]")
    head = ["\t".join([""] + [str(g) for g in genomes]) + "\n"]
    _write_lines(f, head + ["\t".join([str(g)] + [rust_f32(v) for v in row]) + "\n" for g, row in zip(genomes, ani)])


class ClusterValidation(Validation):
    """validate_clusters' result: Validation's counts and records (indices
    into .genomes, the distinct paths of the file in order of appearance),
    the violations with their paths, and .ok.  .n_cached: genomes whose sketch
    came from the sketch cache."""

    def __init__(self, v, clusters, genomes, n_cached):
        self.__dict__.update(v.__dict__)
        self.clusters, self.genomes, self.n_cached = clusters, genomes, n_cached

    def _with_paths(self, pairs, ani):
        return [(self.genomes[int(p["i"])], self.genomes[int(p["j"])], np.float32(a)) for p, a in zip(pairs, ani)]

    @property
    def member_violation_paths(self):
        """[(representative path, member path, f32 ANI)]"""
        return self._with_paths(*self.member_violations)

    @property
    def rep_violation_paths(self):
        """[(representative path, representative path, f32 ANI)]"""
        return self._with_paths(*self.rep_violations)


def validate_clusters(clustering_file, ani_threshold, num_kmers=1000, kmer_length=21, sketch_cache_dir=None):
    """src/cluster_validation.rs:7-78 (galah cluster-validate) with finch's ANI
    in FastANI's place: reads the cluster definition file, sketches every
    distinct path once, checks every member against its representative
    (>= ani_threshold) and every pair of representatives (< ani_threshold) on
    the GPU -> ClusterValidation.  ani_threshold is a fraction (f32).  Logs
    the reference's lines on the "galah" logger with "finch ANI" for
    "FastANI" and the values as it prints them (percent: ani * 100 in f32):
    "not ok" at error level, "ok" at debug level (the pairs in file order; a
    representative against itself is not compared).  At debug level every
    pair's value is fetched for those lines."""
    log = logging.getLogger("galah")
    thr = np.float32(ani_threshold)
    named = read_clustering_file(clustering_file)
    log.info("Read in %d clusters", len(named))  # :17
    if log.isEnabledFor(logging.DEBUG):
        log.debug("Clusters were: %s", _rust_pretty(named))  # :18
    index, genomes = {}, []
    for c in named:
        for p in c:
            if p not in index:
                index[p] = len(genomes)
                genomes.append(p)
    clusters = [[index[p] for p in c] for c in named]
    with _sketching():
        ctx = _context(int(kmer_length), int(num_kmers))
        sk, lens, n_cached = ctx.sketch_files(genomes, cache_dir=sketch_cache_dir)
        v = ctx.validate_clusters(sk, lens, clusters, float(thr))
    out = ClusterValidation(v, clusters, genomes, n_cached)
    hundred = np.float32(100)
    if log.isEnabledFor(logging.DEBUG):
        member_list = [(c[0], g) for c in clusters for g in c[1:] if g != c[0]]
        rep_list = [(clusters[a][0], clusters[b][0]) for a in range(len(clusters)) for b in range(a + 1, len(clusters))]
        _, ani = ctx.ani_pairs(sk, lens, member_list + rep_list) if member_list or rep_list else (None, [])
        for (r, g), a in zip(member_list, ani):
            if np.float32(a) >= thr:
                log.debug("finch ANI between %s and %s is ok: %s", genomes[r], genomes[g],
                          rust_f32(np.float32(a) * hundred))
        for (r1, r2), a in zip(rep_list, ani[len(member_list):]):
            if np.float32(a) < thr:
                log.debug("finch ANI between reps %s and %s is ok: %s", genomes[r1], genomes[r2],
                          rust_f32(np.float32(a) * hundred))
    for r, g, a in out.member_violation_paths:  # :31-34
        log.error("finch ANI between %s and %s is not ok: %s", r, g, rust_f32(a * hundred))
    for r1, r2, a in out.rep_violation_paths:  # :62-65
        log.error("finch ANI between reps %s and %s is not ok: %s", r1, r2, rust_f32(a * hundred))
    return out


def _rust_pretty(clusters):
    """Rust's `{:#?}` of a Vec<Vec<String>>."""
    if not clusters:
        return "[]"
    out = ["["]
    for c in clusters:
        out.append("    [")
        out.extend("        %s," % _rust_str_debug(p) for p in c)
        out.append("    ],")
    out.append("]")
    return "\n".join(out)
