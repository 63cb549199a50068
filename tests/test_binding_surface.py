"""The Python binding's surface and its host forms, pinned before the binding's
call frame was shared.  No device is needed.

The tables below were taken from galah_amd/__init__.py as it stood at commit
68eb3f2, before any wrapper moved: every public method of the eight classes
with its signature, every public module name (and every private one that the
tests, bench.py, __graft_entry__.py or scripts/*.py read) and, for every
function of EXPORTED_SYMBOLS, its restype and argtypes.  The same file passes
on that commit's module and on this tree's.

The refusals: every status and every message was read from the library's
source (the set_thread_error() / fail() texts of pack.cpp, precluster.cpp,
cluster.cpp, border.cpp, query.cpp, sketch_cache.cpp, api.cpp and the
check_*() helpers of ani_pairs.hip and ani_matrix.hip), and every class, dtype
and shape from that commit's Python; nothing was taken from what a run printed.
A refusal is followed by a small valid call of the same wrapper.  Wrappers of
the list in the issue for which Python's own argument handling leaves no
refusal of the library reachable: none; each has one below.
"""
import ctypes
import importlib.util
import inspect
import os
import types

import numpy as np
import pytest

import galah_amd as ga
import oracle

INVALID, IO = 1, 2
K = 21
NAN = float("nan")

SIGNATURES = {
    "gg_abi_version": "u32",
    "gg_status_string": "str i32",
    "gg_last_error": "str vp",
    "gg_thread_last_error": "str",
    "gg_create": "vp i32 u32 u64 i32 Pi32",
    "gg_destroy": "void vp",
    "gg_device": "i32 vp",
    "gg_pack_files": "i32 Pstr u32 i32 i32 PP_Packed",
    "gg_pack_records": "i32 Pvp vp vp u64 u32 i32 PP_Packed",
    "gg_packed_free": "void P_Packed",
    "gg_sketch": "i32 vp P_Packed vp vp",
    "gg_sketch_device": "i32 vp vp u64 vp u64 u32 vp vp vp",
    "gg_pair_tiles": "u64 u32",
    "gg_pair_partition": "void u32 u32 u32 Pu64 Pu64",
    "gg_pairs": "i32 vp vp vp u32 f32 Pvp Pu64",
    "gg_pairs_device": "i32 vp vp vp u32 u64 u64 f32 vp u64 vp vp",
    "gg_precluster_files": "i32 vp Pstr u32 f32 Pvp Pvp Pu64",
    "gg_ani_f64": "f64 u32 u32 i32",
    "gg_ani_f32": "f32 u32 u32 i32",
    "gg_parse_percentage": "i32 f32 Pf32",
    "gg_free": "void vp",
    "gg_synth_clustered_device": "i32 vp u32 u32 u32 u32 f32 u64 vp vp vp",
    "gg_timing_enable": "i32 vp i32",
    "gg_timing_read": "i32 vp i32 P_KStats",
    "gg_pair_paths": "i32 vp vp",
    "gg_partition_preclusters": "i32 u32 vp u64 vp vp Pu32",
    "gg_precluster_pairs": "i32 u32 vp u64 vp vp u32 vp vp",
    "gg_synth_mixed_lengths": "i32 u32 u32 u32 u32 u32 u64 vp",
    "gg_synth_mixed_device": "i32 vp u32 u32 vp u32 f32 f64 u64 vp vp u64 Pu64 vp",
    "gg_sketch_cache_load": "i32 str str i32 u32 u64 vp Pu32 Pi32",
    "gg_sketch_cache_store": "i32 str str i32 u32 u64 vp u32",
    "gg_sketch_files": "i32 vp Pstr u32 str vp vp Pu32",
    "gg_precluster_files_cached": "i32 vp Pstr u32 f32 str Pvp Pvp Pu64 Pu32",
    "gg_create_multi": "vp i32 u32 u64 vp u32 Pi32",
    "gg_device_count": "u32 vp",
    "gg_device_ctx": "vp vp u32",
    "gg_set_host_threads": "i32 vp i32",
    "gg_phase_times": "i32 vp vp",
    "gg_precluster_shards": "i32 vp vp f32 Pvp Pvp Pu64",
    "gg_fallbacks": "i32 vp vp",
    "gg_peer_links": "i32 vp vp",
    "gg_info_line": "i32 vp str u64",
    "gg_precluster_files_each": "i32 vp Pstr u32 f32 str fn(i32:vp,vp,u64) vp Pvp Pvp Pu64 Pu32",
    "gg_genome_stats_files": "i32 Pstr u32 i32 vp",
    "gg_sketch_files_stats": "i32 vp Pstr u32 str vp vp vp",
    "gg_cluster_pairs_host": "i32 u32 vp vp u64 f32 vp",
    "gg_cluster_pairs": "i32 vp u32 vp vp u64 f32 vp",
    "gg_cluster_pairs_device": "i32 vp u32 vp vp u64 f32 vp vp",
    "gg_clusters_from_reps": "i32 u32 vp vp vp Pu32",
    "gg_cluster_files": "i32 vp Pstr u32 f32 f32 str vp Pvp Pvp Pu64",
    "gg_ani_pairs_host": "i32 vp vp u32 u32 i32 vp u64 vp",
    "gg_ani_pairs": "i32 vp vp vp u32 vp u64 vp",
    "gg_ani_pairs_device": "i32 vp vp vp u32 vp u64 vp",
    "gg_validate_clusters_host": "i32 vp vp u32 u32 i32 vp vp u32 f32 P_Validation Pvp Pvp Pu64",
    "gg_validate_clusters": "i32 vp vp vp u32 vp vp u32 f32 P_Validation Pvp Pvp Pu64",
    "gg_validate_files": "i32 vp Pstr u32 vp vp u32 f32 str P_Validation Pvp Pvp Pu64",
    "gg_pairs_border": "i32 vp vp vp u32 u32 f32 Pvp Pu64",
    "gg_pairs_border_device": "i32 vp vp vp u32 u32 f32 vp u64 vp vp",
    "gg_pairs_border_host": "i32 vp vp u32 u32 u32 i32 f32 Pvp Pu64",
    "gg_update_files": "i32 vp vp vp u32 Pstr u32 f32 str vp vp Pvp Pvp Pu64",
    "gg_preclusters": "i32 vp u32 vp u64 vp vp Pu32 vp vp",
    "gg_preclusters_device": "i32 vp u32 vp u64 vp vp Pu32 vp vp vp",
    "gg_ani_f32_device": "i32 vp vp u64 vp vp Pu64 vp",
    "gg_cluster_rows_device": "i32 vp vp vp u32 f32 f32 vp P_ClusterSummary Pvp Pvp vp",
    "gg_cluster_files_resident": "i32 vp Pstr u32 f32 f32 str vp P_ClusterSummary",
    "gg_ani_matrix_host": "i32 vp vp u32 u32 i32 vp u32 vp vp vp",
    "gg_ani_matrix": "i32 vp vp vp u32 vp u32 vp vp vp P_MatrixSummary",
    "gg_ani_matrix_device": "i32 vp vp vp u32 vp u32 vp vp vp P_MatrixSummary vp",
    "gg_ani_matrix_files": "i32 vp Pstr u32 str vp vp vp P_MatrixSummary",
    "gg_ani_matrix_group_cells": "i32 vp u32 vp",
    "gg_ani_matrix_groups_host": "i32 vp vp u32 u32 i32 vp vp u32 vp vp vp",
    "gg_ani_matrix_groups": "i32 vp vp vp u32 vp vp u32 vp vp vp P_MatrixSummary",
    "gg_ani_matrix_groups_device": "i32 vp vp vp u32 vp vp u32 vp vp vp P_MatrixSummary vp",
    "gg_precluster_matrices_files": "i32 vp Pstr u32 f32 str Pvp Pvp Pu32 Pvp Pvp Pvp Pvp P_MatrixSummary",
    "gg_pairs_matrix_device": "i32 vp vp vp u32 vp u32 f32 vp u64 vp P_PairsMatrixSummary vp",
    "gg_pairs_matrix": "i32 vp vp vp u32 vp u32 f32 Pvp Pu64 P_PairsMatrixSummary",
    "gg_pairs_border_matrix_device": "i32 vp vp vp u32 u32 f32 vp u64 vp P_PairsMatrixSummary vp",
    "gg_pairs_border_matrix": "i32 vp vp vp u32 u32 f32 Pvp Pu64 P_PairsMatrixSummary",
    "gg_set_pairs_path": "i32 vp i32",
    "gg_pairs_path": "i32 vp",
    "gg_pairs_paths_taken": "i32 vp vp",
    "gg_precluster_files_resident": "i32 vp Pstr u32 f32 str Pvp Pvp Pu64 P_PairsMatrixSummary",
    "gg_collection_create": "i32 vp f32 u32 u64 Pvp",
    "gg_collection_destroy": "void vp",
    "gg_collection_stat": "i32 vp P_CollectionInfo Pf32",
    "gg_collection_load": "i32 vp vp vp u32 vp vp u64 f32 Pvp",
    "gg_collection_add_rows": "i32 vp vp vp u32 Pu64",
    "gg_collection_add_rows_device": "i32 vp vp vp u32 Pu64 vp",
    "gg_collection_add_files": "i32 vp Pstr u32 str Pu64",
    "gg_collection_remove": "i32 vp vp u32 vp",
    "gg_collection_cluster": "i32 vp vp f32 vp",
    "gg_collection_pairs": "i32 vp Pvp Pvp Pu64",
    "gg_collection_rows": "i32 vp vp vp",
    "gg_collection_view": "i32 vp Pvp Pvp Pvp Pvp",
    "gg_query_host": "i32 vp vp u32 vp vp u32 u32 i32 f32 Pvp Pu64",
    "gg_query_rows": "i32 vp vp vp u32 vp vp u32 f32 Pvp Pvp Pu64",
    "gg_query_rows_device": "i32 vp vp vp u32 vp vp u32 f32 vp u64 vp vp",
    "gg_query_best_host": "i32 u32 u32 vp vp u64 vp vp vp",
    "gg_query_best_device": "i32 vp u32 u32 vp vp u64 vp vp vp vp",
    "gg_collection_query_rows": "i32 vp vp vp u32 f32 Pvp Pvp Pu64",
    "gg_collection_query_files": "i32 vp Pstr u32 str f32 vp vp Pvp Pvp Pu64",
    "gg_collection_classify_rows": "i32 vp vp vp u32 vp vp vp",
    "gg_collection_classify_files": "i32 vp Pstr u32 str vp vp vp",
}

# the structs the signatures name, field by field
STRUCTS = {
    "_ClusterSummary": "n_pairs:u64 ani_rechecked:u64 n_preclusters:u32 largest_precluster:u32 pair_passes:u32 reserved:u32",
    "_CollectionInfo": "n_pairs:u64 pair_capacity:u64 device_bytes:u64 n_rows:u32 row_capacity:u32 grows:u32 rows_moved:u32",
    "_KStats": "ms:f64 launches:u64 work:u64",
    "_MatrixSummary": "n_entries:u64 n_columns:u64 column_entries:u64 ani_rechecked:u64",
    "_Packed": "words:Pu32 n_words:u64 n_bases:u64 runs:P_Run n_runs:u64 n_genomes:u32 genome_kmers:Pu64",
    "_PairsMatrixSummary": "n_entries:u64 n_columns:u64 column_entries:u64 n_pairs:u64 chunk_rounds:u64 index_reads:u64 "
                           "path:u32 pair_passes:u32",
    "_Run": "genome:u32 len:u32 base:u64",
    "_Validation": "member_pairs:u64 member_bad:u64 rep_pairs:u64 rep_bad:u64",
}

DEV = "(self, d_sketches, d_lens, n, "
CLASSES = {
    "Context": {
        "__init__": "(self, k=21, sketch_size=1000, seed=0, device=-1, devices=None, host_threads=0)",
        "ani_f32_device": "(self, d_pairs, n_pairs, d_ani, d_ani_f64=None, stream=None)",
        "ani_matrix": "(self, sketches, lens, rows=None)",
        "ani_matrix_device": DEV + "d_rows, m, d_common=None, d_total=None, d_ani=None, stream=None)",
        "ani_matrix_files": "(self, paths, cache_dir=None)",
        "ani_matrix_groups": "(self, sketches, lens, members, offsets=None)",
        "ani_matrix_groups_device": DEV + "d_members, offsets, d_common=None, d_total=None, d_ani=None, stream=None)",
        "ani_pairs": "(self, sketches, lens, pairs)",
        "ani_pairs_device": DEV + "d_list, m, stream=None)",
        "close": "(self)",
        "cluster_files": "(self, paths, min_ani, cluster_ani, cache_dir=None, want_pairs=True)",
        "cluster_files_resident": "(self, paths, min_ani, cluster_ani, cache_dir=None)",
        "cluster_pairs": "(self, n_genomes, pairs, ani, cluster_ani)",
        "cluster_pairs_device": "(self, n_genomes, d_pairs, d_ani, n_pairs, cluster_ani, d_rep_of, stream=None)",
        "cluster_rows_device": DEV + "min_ani, cluster_ani, d_rep_of, want_summary=True, stream=None)",
        "collection_add_files": "(self, handle, paths, cache_dir=None)",
        "collection_add_rows": "(self, handle, sketches, lens)",
        "collection_add_rows_device": "(self, handle, d_sketches, d_lens, n_new, stream=None)",
        "collection_classify_files": "(self, handle, paths, rank=None, cache_dir=None)",
        "collection_classify_rows": "(self, handle, q_sketches, q_lens, rank=None)",
        "collection_cluster": "(self, handle, cluster_ani, order=None)",
        "collection_create": "(self, min_ani, reserve_rows=0, reserve_pairs=0)",
        "collection_destroy": "(self, handle)",
        "collection_load": "(self, sketches, lens, pairs, ani, min_ani)",
        "collection_pairs": "(self, handle)",
        "collection_query_files": "(self, handle, paths, min_ani, cache_dir=None, want_sketches=False)",
        "collection_query_rows": "(self, handle, q_sketches, q_lens, min_ani)",
        "collection_remove": "(self, handle, rows)",
        "collection_rows": "(self, handle)",
        "collection_stat": "(self, handle)",
        "collection_view": "(self, handle)",
        "device": "property",
        "device_count": "property",
        "fallbacks": "(self)",
        "info_line": "(self)",
        "member": "(self, i)",
        "pair_paths": "(self)",
        "pairs": "(self, sketches, lens, min_ani)",
        "pairs_border": "(self, sketches, lens, n_old, min_ani)",
        "pairs_border_device": DEV + "n_old, min_ani, d_out, out_cap, d_count, stream=None)",
        "pairs_border_matrix": "(self, sketches, lens, n_old, min_ani)",
        "pairs_border_matrix_device": DEV + "n_old, min_ani, d_out, out_cap, d_count, want_summary=True, stream=None)",
        "pairs_device": DEV + "tile_begin, tile_end, min_ani, d_out, out_cap, d_count, stream=None)",
        "pairs_matrix": "(self, sketches, lens, min_ani, rows=None)",
        "pairs_matrix_device": DEV + "d_rows, m, min_ani, d_out, out_cap, d_count, want_summary=True, stream=None)",
        "pairs_path": "property",
        "pairs_paths_taken": "(self)",
        "peer_links": "(self)",
        "phase_times": "(self)",
        "precluster_files": "(self, paths, min_ani, cache_dir=None)",
        "precluster_files_each": "(self, paths, min_ani, each, cache_dir=None)",
        "precluster_files_resident": "(self, paths, min_ani, cache_dir=None)",
        "precluster_matrices_files": "(self, paths, min_ani, cache_dir=None)",
        "precluster_shards": "(self, shards, min_ani)",
        "preclusters": "(self, n_genomes, pairs, with_pairs=True)",
        "preclusters_device": "(self, n_genomes, d_pairs, n_pairs, d_members, d_offsets, d_local=None, "
                              "d_pair_offsets=None, stream=None)",
        "query_best_device": "(self, n, nq, d_pairs, d_ani, n_pairs, d_rank, d_best, d_best_ani, stream=None)",
        "query_rows": "(self, sketches, lens, q_sketches, q_lens, min_ani)",
        "query_rows_device": DEV + "d_q_sketches, d_q_lens, nq, min_ani, d_out, out_cap, d_count, stream=None)",
        "set_host_threads": "(self, n)",
        "set_pairs_path": "(self, path)",
        "sketch": "(self, packed)",
        "sketch_device": "(self, d_words, runs, n_genomes, d_out, d_lens, stream=None)",
        "sketch_files": "(self, paths, cache_dir=None)",
        "sketch_files_stats": "(self, paths, cache_dir=None)",
        "synth_device": "(self, n_genomes, genome_len, cluster_size, max_sub_rate, seed, d_words, stream=None, "
                        "first_genome=0)",
        "synth_mixed_device": "(self, lens, cluster_size, max_sub_rate, n_run_rate, seed, d_words, stream=None, "
                              "first_genome=0)",
        "timing_enable": "(self, on=True)",
        "timing_read": "(self, kernel)",
        "update_files": "(self, old_sketches, old_lens, new_paths, min_ani, cache_dir=None)",
        "validate_clusters": "(self, sketches, lens, clusters, ani)",
        "validate_files": "(self, paths, clusters, ani, cache_dir=None)",
    },
    "Collection": {
        "__init__": "(self, preclusterer, reserve=0, _handle=None, _paths=())",
        "add": "(self, paths)",
        "cache": "(self)",
        "classify": "(self, paths, clusterer, order=None)",
        "close": "(self)",
        "cluster": "(self, clusterer, order=None)",
        "from_state": "classmethod(cls, state, preclusterer)",
        "info": "(self)",
        "paths": "property",
        "query": "(self, paths, min_ani=None)",
        "remove": "(self, paths)",
        "state": "(self)",
    },
    "FinchPreclusterer": {
        "__init__": "(self, min_ani, num_kmers=1000, kmer_length=21, sketch_cache_dir=None, pairs_path=None)",
        "collection": "(self, reserve=0)",
        "distances": "(self, genome_fasta_paths)",
        "distances_state": "(self, genome_fasta_paths)",
        "method_name": "(self)",
        "update": "(self, state, new_paths)",
    },
    "FinchClusterer": {
        "__init__": "(self, ani, num_kmers=1000, kmer_length=21)",
        "calculate_ani": "(self, fasta1, fasta2)",
        "calculate_ani_many": "(self, pairs_of_paths, sketch_cache_dir=None)",
        "get_ani_threshold": "(self)",
        "initialise": "(self)",
        "method_name": "(self)",
    },
    "PreclusterState": {
        "__init__": "(self, paths, sketches, lens, pairs, ani, k, s, seed, min_ani)",
        "cache": "(self)",
        "load": "classmethod(cls, file)",
        "save": "(self, file)",
    },
    "Packed": {
        "__init__": "(self, ptr)",
        "free": "(self)",
    },
    "Validation": {
        "__init__": "(self, summary, bad, bad_ani)",
        "member_violations": "property",
        "ok": "property",
        "rep_violations": "property",
    },
    "SortedPairGenomeDistanceCache": {
        "__init__": "(self)",
        "contains_key": "(self, genome_ids)",
        "get": "(self, genome_ids)",
        "insert": "(self, genome_ids, distance)",
        "transform_ids": "(self, input_ids)",
    },
}

# every public module name, and the private ones read from outside the module
MODULE = {
    "ClusterDistanceFinder": "class",
    "ClusterValidation": "class",
    "Collection": "class",
    "Context": "class",
    "EXPORTED_SYMBOLS": "value",
    "FALLBACKS": "value",
    "FinchClusterer": "class",
    "FinchPreclusterer": "class",
    "GG_ERR_NO_DEVICE": "value",
    "GG_OK": "value",
    "GG_PAIR_TILE": "value",
    "GalahGpuError": "class",
    "GenomeAssemblyStats": "class",
    "HERE": "value",
    "INGEST_KERNELS": "value",
    "KERNEL_ANI_PAIRS": "value",
    "KERNEL_CLUSTER": "value",
    "KERNEL_FINALIZE": "value",
    "KERNEL_INFLATE_CRC": "value",
    "KERNEL_INFLATE_DECODE": "value",
    "KERNEL_INFLATE_EXPAND": "value",
    "KERNEL_INFLATE_RESOLVE": "value",
    "KERNEL_INFLATE_SEARCH": "value",
    "KERNEL_PAIRS": "value",
    "KERNEL_PAIRS_INDEX": "value",
    "KERNEL_PARSE": "value",
    "KERNEL_PRECLUSTER": "value",
    "KERNEL_SKETCH": "value",
    "KERNEL_UPLOAD": "value",
    "LIB_PATH": "value",
    "LOCAL_PAIR_DTYPE": "value",
    "MISSING": "value",
    "PAIRS_PATHS": "value",
    "PAIR_DTYPE": "value",
    "PAIR_SINK": "class",
    "PHASES": "value",
    "Packed": "class",
    "PreclusterDistanceFinder": "class",
    "PreclusterState": "class",
    "RUN_DTYPE": "value",
    "STATS_DTYPE": "value",
    "SortedPairGenomeDistanceCache": "class",
    "Validation": "class",
    "_ClusterSummary": "class",
    "_CollectionInfo": "class",
    "_KStats": "class",
    "_L": "value",
    "_MatrixSummary": "class",
    "_Packed": "class",
    "_PairsMatrixSummary": "class",
    "_Run": "class",
    "_Validation": "class",
    "_context": "def(k, s, seed=0)",
    "_ptr": "def(a)",
    "abi_version": "def()",
    "ani_f32": "def(common, total, k=21)",
    "ani_f64": "def(common, total, k=21)",
    "ani_matrix": "def(genomes, num_kmers=1000, kmer_length=21, sketch_cache_dir=None)",
    "ani_matrix_block": "def(values, offsets, cell_offsets, g)",
    "ani_matrix_group_cells": "def(offsets)",
    "ani_matrix_groups_host": "def(sketches, lens, members, offsets=None, k=21)",
    "ani_matrix_host": "def(sketches, lens, rows=None, k=21)",
    "ani_pairs_host": "def(sketches, lens, pairs, k=21)",
    "calculate_genome_stats": "def(fasta_path)",
    "cluster": "def(genomes, preclusterer, clusterer, sketch_cache_dir=None)",
    "cluster_pairs_host": "def(n_genomes, pairs, ani, cluster_ani)",
    "cluster_update": "def(state, new_paths, preclusterer, clusterer, order=None)",
    "clusters_from_reps": "def(rep_of)",
    "device_runs": "def(runs, device)",
    "distances": "def(genome_fasta_paths, min_ani, num_kmers, kmer_length, sketch_cache_dir=None, pairs_path=None)",
    "genome_stats": "def(paths, threads=0)",
    "lib": "def()",
    "pack_files": "def(paths, k=21, threads=0)",
    "pack_records": "def(genomes, k=21)",
    "pair_partition": "def(n, parts, part)",
    "pair_tiles": "def(n)",
    "pairs_border_host": "def(sketches, lens, n_old, min_ani, k=21)",
    "parse_percentage": "def(value)",
    "partition_preclusters": "def(n_genomes, pairs)",
    "precluster_ani_matrices": "def(genomes, precluster_ani=0.9, num_kmers=1000, kmer_length=21, sketch_cache_dir=None)",
    "precluster_pairs": "def(n_genomes, pairs, members, offsets)",
    "preclusters": "def(n_genomes, pairs)",
    "query_best_host": "def(n, nq, pairs, ani, rank=None)",
    "query_host": "def(sketches, lens, q_sketches, q_lens, min_ani, k=21)",
    "read_clustering_file": "def(path)",
    "relabel_pairs": "def(pairs, order)",
    "rust_f32": "def(x)",
    "rust_f64": "def(x)",
    "sketch_cache_load": "def(cache_dir, path, k=21, s=1000, seed=0)",
    "sketch_cache_store": "def(cache_dir, path, hashes, k=21, s=1000, seed=0)",
    "synth_mixed_lengths": "def(n_genomes, min_len, max_len, cluster_size, seed, first_genome=0)",
    "validate_clusters": "def(clustering_file, ani_threshold, num_kmers=1000, kmer_length=21, sketch_cache_dir=None)",
    "validate_clusters_host": "def(sketches, lens, clusters, ani, k=21)",
    "write_ani_matrix": "def(f, genomes, ani)",
    "write_cluster_definition": "def(f, clusters, genomes)",
    "write_representative_list": "def(f, clusters, genomes)",
}

VALUES = {
    "FALLBACKS": ("index_to_gate", "index_full_sort", "peer_staged", "sketch_retry", "inflate_host", "sketch_set"),
    "GG_ERR_NO_DEVICE": 4, "GG_OK": 0, "GG_PAIR_TILE": 64,
    "INGEST_KERNELS": {"search": 4, "decode": 5, "expand": 6, "resolve": 7, "crc": 8, "parse": 9, "upload": 10},
    "KERNEL_SKETCH": 0, "KERNEL_FINALIZE": 1, "KERNEL_PAIRS": 2, "KERNEL_PAIRS_INDEX": 3, "KERNEL_INFLATE_SEARCH": 4,
    "KERNEL_INFLATE_DECODE": 5, "KERNEL_INFLATE_EXPAND": 6, "KERNEL_INFLATE_RESOLVE": 7, "KERNEL_INFLATE_CRC": 8,
    "KERNEL_PARSE": 9, "KERNEL_UPLOAD": 10, "KERNEL_CLUSTER": 11, "KERNEL_ANI_PAIRS": 12, "KERNEL_PRECLUSTER": 13,
    "PAIRS_PATHS": ("default", "matrix", "auto"),
    "PHASES": ("sketch", "replicate", "pairs", "merge"),
    "PAIR_DTYPE": np.dtype([("i", "<u4"), ("j", "<u4"), ("common", "<u4"), ("total", "<u4")]),
    "LOCAL_PAIR_DTYPE": np.dtype([("precluster", "<u4"), ("i", "<u4"), ("j", "<u4"), ("src", "<u4")]),
    "RUN_DTYPE": np.dtype([("genome", "<u4"), ("len", "<u4"), ("base", "<u8")]),
    "STATS_DTYPE": np.dtype([("num_contigs", "<u8"), ("num_ambiguous_bases", "<u8"), ("n50", "<u8"),
                             ("total_bases", "<u8")]),
}

ALL = [
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

# (c_size_t is c_uint64 here: one name for both)
SHORT = {ctypes.c_void_p: "vp", ctypes.c_uint32: "u32", ctypes.c_uint64: "u64", ctypes.c_int: "i32",
         ctypes.c_float: "f32", ctypes.c_double: "f64", ctypes.c_char_p: "str"}


def tname(t):
    """A ctypes type spelled by value: simple types by width, P<pointee>, fn(restype:argtypes), a struct by its name."""
    if t is None:
        return "void"
    if t in SHORT:
        return SHORT[t]
    if hasattr(t, "_type_") and not isinstance(t._type_, str):
        return "P" + tname(t._type_)
    if hasattr(t, "_argtypes_"):
        return "fn(%s:%s)" % (tname(t._restype_), ",".join(tname(a) for a in t._argtypes_))
    return t.__name__


def members(cls):
    out = {}
    for name, v in vars(cls).items():
        if name.startswith("_") and name != "__init__":
            continue
        if isinstance(v, property):
            out[name] = "property"
        elif isinstance(v, (staticmethod, classmethod)):
            out[name] = type(v).__name__ + str(inspect.signature(v.__func__))
        elif callable(v):
            out[name] = str(inspect.signature(v))
        else:
            out[name] = "value"
    return out


def describe(v):
    if isinstance(v, type):
        return "class"
    if callable(v):
        return "def" + str(inspect.signature(v))
    return "value"


# ---- the surface ---------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_class_surface(cls):
    got = members(getattr(ga, cls))
    assert sorted(got) == sorted(CLASSES[cls])  # none missing, none new
    for name, sig in CLASSES[cls].items():
        assert got[name] == sig, name


def test_module_surface():
    public = sorted(n for n in dir(ga) if not n.startswith("_") and not isinstance(getattr(ga, n), types.ModuleType))
    assert public == sorted(n for n in MODULE if not n.startswith("_"))  # none missing, none new
    for name, what in MODULE.items():
        assert describe(getattr(ga, name)) == what, name
    assert ga.ctypes is ctypes  # (read through the module by a test)
    for name, value in VALUES.items():
        assert getattr(ga, name) == value and type(getattr(ga, name)) is type(value), name
    assert ga.__all__ == ALL and all(hasattr(ga, n) for n in ALL)
    assert ga.lib() is ga._L and ga.LIB_PATH == ga._L._name
    assert ga.MISSING is not None and issubclass(ga.GalahGpuError, RuntimeError)
    assert issubclass(ga.ClusterValidation, ga.Validation) and issubclass(ga.FinchPreclusterer, ga.PreclusterDistanceFinder)
    assert issubclass(ga.FinchClusterer, ga.ClusterDistanceFinder)


def test_signature_table():
    assert sorted(ga.EXPORTED_SYMBOLS) == sorted(SIGNATURES) and len(set(ga.EXPORTED_SYMBOLS)) == len(SIGNATURES)
    for name in ga.EXPORTED_SYMBOLS:
        f = getattr(ga._L, name)
        assert " ".join([tname(f.restype)] + [tname(a) for a in f.argtypes]) == SIGNATURES[name], name
    for name, fields in STRUCTS.items():
        assert " ".join("%s:%s" % (f, tname(t)) for f, t in getattr(ga, name)._fields_) == fields, name


def test_summary_dicts():
    """as_dict of the four summary structs: every field as an int, `reserved` dropped, `path` by its name."""
    for name, fields in STRUCTS.items():
        if name in ("_ClusterSummary", "_CollectionInfo", "_MatrixSummary", "_PairsMatrixSummary"):
            d = getattr(ga, name)().as_dict()
            assert list(d) == [f.split(":")[0] for f in fields.split() if not f.startswith("reserved:")]
            assert all(type(v) is int and v == 0 for k, v in d.items() if k != "path")
    s = ga._PairsMatrixSummary()
    assert s.as_dict()["path"] == "default"
    s.path, s.n_pairs = 1, 7
    assert s.as_dict()["path"] == "matrix" and s.as_dict()["n_pairs"] == 7


# ---- the module as a plain module over a library named by GALAHGPU_LIB ---------------
ROWS = np.array([[1, 2, 3, 4], [1, 2, 3, 5]], np.uint64)
LENS = np.array([4, 4], np.uint32)


def expected_pair(sk, lens, i, j):
    c, t = oracle.raw_distance(sk[i][:lens[i]], sk[j][:lens[j]])
    return int(c), int(t), ga.ani_f32(int(c), int(t), K)


def test_second_module_over_named_library():
    lib = ga.LIB_PATH  # the product library, named by GALAHGPU_LIB as tests/conftest.py names the cross-check build
    spec = importlib.util.spec_from_file_location("galah_amd_second", os.path.join(os.path.dirname(ga.__file__), "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    old = os.environ.get("GALAHGPU_LIB")
    os.environ["GALAHGPU_LIB"] = lib
    try:
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            os.environ.pop("GALAHGPU_LIB")
        else:
            os.environ["GALAHGPU_LIB"] = old
    assert mod._L is not ga._L and mod.lib() is mod._L
    assert mod.LIB_PATH == lib and mod._L._name == lib
    assert mod.Context is not ga.Context and mod.GalahGpuError is not ga.GalahGpuError
    p, ani = mod.ani_pairs_host(ROWS, LENS, [(0, 1)])
    c, t, a = expected_pair(ROWS, LENS, 0, 1)
    assert (int(p["common"][0]), int(p["total"][0])) == (c, t) and ani.tolist() == [a]
    with pytest.raises(mod.GalahGpuError) as e:  # its own error class, its own library's thread error
        mod.ani_pairs_host(ROWS, LENS, [(0, 2)])
    assert str(e.value) == "gg_ani_pairs_host: pair index out of range (status 1)"


# ---- a refusal, then a valid call, of every host wrapper ----------------------------
def refused(status, text, fn, *args, **kw):
    with pytest.raises(ga.GalahGpuError) as e:
        fn(*args, **kw)
    assert type(e.value) is ga.GalahGpuError and e.value.status == status
    assert str(e.value) == "%s (status %d)" % (text, status)


def pair_list(ij):
    p = np.zeros(len(ij), ga.PAIR_DTYPE)
    for x, (i, j) in enumerate(ij):
        p[x]["i"], p[x]["j"] = i, j
    return p


def test_synth_mixed_lengths():
    refused(INVALID, "gg_synth_mixed_lengths: bad arguments", ga.synth_mixed_lengths, 3, 32, 128, 2, 1)  # min_len < 64
    lens = ga.synth_mixed_lengths(3, 64, 128, 2, 1)
    assert lens.dtype == np.uint32 and lens.shape == (3,) and ((lens >= 64) & (lens <= 128)).all()
    assert lens[0] == lens[1]  # (one length per cluster of 2)
    empty = ga.synth_mixed_lengths(0, 64, 128, 2, 1)
    assert empty.dtype == np.uint32 and empty.shape == (0,)


def test_partition_preclusters_and_precluster_pairs():
    refused(INVALID, "gg_partition_preclusters: pair index out of range", ga.partition_preclusters, 3, pair_list([(0, 3)]))
    members, offsets = ga.partition_preclusters(3, pair_list([(1, 2)]))
    assert members.tolist() == [1, 2, 0] and offsets.tolist() == [0, 2, 3]
    assert members.dtype == offsets.dtype == np.uint32
    refused(INVALID, "gg_precluster_pairs: pair is not inside one precluster", ga.precluster_pairs, 3,
            pair_list([(0, 1)]), members, offsets)
    refused(INVALID, "gg_precluster_pairs: bad offsets", ga.precluster_pairs, 3, pair_list([(1, 2)]), members, [0, 4, 3])
    local, poff = ga.precluster_pairs(3, pair_list([(1, 2)]), members, offsets)
    assert local.dtype == ga.LOCAL_PAIR_DTYPE and poff.dtype == np.uint64
    assert local.tolist() == [(0, 0, 1, 0)] and poff.tolist() == [0, 1, 1]
    assert ga.preclusters(3, pair_list([(1, 2)])) == [[1, 2], [0]]
    # no genome, no pair
    members, offsets = ga.partition_preclusters(0, pair_list([]))
    assert (members.dtype, members.shape, offsets.dtype, offsets.tolist()) == (np.uint32, (0,), np.uint32, [0])
    local, poff = ga.precluster_pairs(0, pair_list([]), members, offsets)
    assert (local.dtype, local.shape, poff.dtype, poff.tolist()) == (ga.LOCAL_PAIR_DTYPE, (0,), np.uint64, [0])
    assert ga.preclusters(0, pair_list([])) == []


def test_cluster_pairs_host_and_clusters_from_reps():
    refused(INVALID, "gg_cluster_pairs_host: cluster_ani is NaN", ga.cluster_pairs_host, 3, [(0, 1)], [0.99], NAN)
    with pytest.raises(ValueError, match="^one ani per pair$"):  # (Python's own check comes first)
        ga.cluster_pairs_host(3, [(0, 1)], [0.99, 0.98], 0.95)
    rep = ga.cluster_pairs_host(3, [(0, 1)], [0.99], 0.95)
    assert rep.dtype == np.uint32 and rep.tolist() == [0, 0, 2]
    refused(INVALID, "gg_clusters_from_reps: rep_of does not point at representatives", ga.clusters_from_reps, [1, 2, 2])
    assert ga.clusters_from_reps(rep) == [[0, 1], [2]]
    empty = ga.cluster_pairs_host(0, [], [], 0.95)
    assert empty.dtype == np.uint32 and empty.shape == (0,)
    assert ga.clusters_from_reps([]) == []


def test_ani_pairs_host():
    refused(INVALID, "gg_ani_pairs_host: sketch longer than sketch_size", ga.ani_pairs_host, ROWS, [4, 5], [(0, 1)])
    p, ani = ga.ani_pairs_host(ROWS, LENS, [(1, 0), (0, 0)])
    c, t, a = expected_pair(ROWS, LENS, 1, 0)
    assert p.dtype == ga.PAIR_DTYPE and ani.dtype == np.float32 and p.shape == ani.shape == (2,)
    assert p.tolist() == [(1, 0, c, t), (0, 0, 4, 4)] and ani.tolist() == [a, np.float32(1.0)]
    p, ani = ga.ani_pairs_host(np.zeros((0, 4), np.uint64), np.zeros(0, np.uint32), [])
    assert (p.dtype, p.shape, ani.dtype, ani.shape) == (ga.PAIR_DTYPE, (0,), np.float32, (0,))


def test_ani_matrix_host():
    refused(INVALID, "gg_ani_matrix_host: row index out of range", ga.ani_matrix_host, ROWS, LENS, [0, 2])
    common, total, ani = ga.ani_matrix_host(ROWS, LENS, rows=[1, 0])
    c, t, a = expected_pair(ROWS, LENS, 0, 1)
    assert (common.dtype, total.dtype, ani.dtype) == (np.uint32, np.uint32, np.float32)
    assert common.tolist() == [[4, c], [c, 4]] and total.tolist() == [[4, t], [t, 4]] and ani.tolist() == [[1.0, a], [a, 1.0]]
    for m in ga.ani_matrix_host(ROWS, LENS):
        assert m.shape == (2, 2)
    out = ga.ani_matrix_host(np.zeros((0, 4), np.uint64), np.zeros(0, np.uint32))
    assert [(m.dtype, m.shape) for m in out] == [(np.uint32, (0, 0)), (np.uint32, (0, 0)), (np.float32, (0, 0))]
    out = ga.ani_matrix_host(ROWS, LENS, rows=[])
    assert [(m.dtype, m.shape) for m in out] == [(np.uint32, (0, 0)), (np.uint32, (0, 0)), (np.float32, (0, 0))]


def test_ani_matrix_groups_host():
    refused(INVALID, "gg_ani_matrix_group_cells: offsets[0] is not 0", ga.ani_matrix_group_cells, [1, 2])
    refused(INVALID, "gg_ani_matrix_group_cells: offsets do not ascend", ga.ani_matrix_group_cells, [0, 2, 1])
    cells = ga.ani_matrix_group_cells([0, 2, 3])
    assert cells.dtype == np.uint64 and cells.tolist() == [0, 4, 5]
    assert ga.ani_matrix_group_cells([0]).tolist() == [0]
    refused(INVALID, "gg_ani_matrix_groups_host: row index out of range", ga.ani_matrix_groups_host, ROWS, LENS, [[0, 2]])
    with pytest.raises(ValueError, match="^offsets must have n_groups \\+ 1 entries and end within members$"):
        ga.ani_matrix_groups_host(ROWS, LENS, [0, 1], [0, 3])
    common, total, ani, cells = ga.ani_matrix_groups_host(ROWS, LENS, [[1, 0], [1]])
    c, t, a = expected_pair(ROWS, LENS, 0, 1)
    assert common.tolist() == [4, c, c, 4, 4] and total.tolist() == [4, t, t, 4, 4] and cells.tolist() == [0, 4, 5]
    assert ani.tolist() == [1.0, a, a, 1.0, 1.0]
    assert ga.ani_matrix_block(ani, [0, 2, 3], cells, 0).tolist() == [[1.0, a], [a, 1.0]]
    same = ga.ani_matrix_groups_host(ROWS, LENS, [1, 0, 1], [0, 2, 3])
    assert [x.tolist() for x in same] == [common.tolist(), total.tolist(), ani.tolist(), cells.tolist()]
    # no group
    common, total, ani, cells = ga.ani_matrix_groups_host(ROWS, LENS, [])
    assert [(x.dtype, x.shape) for x in (common, total, ani)] == [(np.uint32, (0,)), (np.uint32, (0,)), (np.float32, (0,))]
    assert cells.dtype == np.uint64 and cells.tolist() == [0]


def test_pairs_border_host():
    refused(INVALID, "gg_pairs_border_host: n_old exceeds n", ga.pairs_border_host, ROWS, LENS, 3, 0.0)
    refused(INVALID, "min_ani is NaN", ga.pairs_border_host, ROWS, LENS, 0, NAN)  # (no prefix: DESIGN.md 4.16)
    c, t, _ = expected_pair(ROWS, LENS, 0, 1)
    pairs = ga.pairs_border_host(ROWS, LENS, 1, 0.0)
    assert pairs.dtype == ga.PAIR_DTYPE and pairs.tolist() == [(0, 1, c, t)]
    for n_old, rows, lens in ((2, ROWS, LENS), (0, np.zeros((0, 4), np.uint64), np.zeros(0, np.uint32))):
        none = ga.pairs_border_host(rows, lens, n_old, 0.0)
        assert none.dtype == ga.PAIR_DTYPE and none.shape == (0,)


def test_query_host_and_query_best_host():
    refused(INVALID, "min_ani is NaN", ga.query_host, ROWS[:1], LENS[:1], ROWS[1:], LENS[1:], NAN)
    refused(INVALID, "gg_query_host: sketch longer than sketch_size", ga.query_host, ROWS[:1], LENS[:1], ROWS[1:], [5], 0.0)
    c, t, a = expected_pair(ROWS, LENS, 0, 1)
    hits = ga.query_host(ROWS[:1], LENS[:1], ROWS[1:], LENS[1:], 0.0)
    assert hits.dtype == ga.PAIR_DTYPE and hits.tolist() == [(0, 1, c, t)]
    empty_rows, empty_lens = np.zeros((0, 4), np.uint64), np.zeros(0, np.uint32)
    for args in ((empty_rows, empty_lens, ROWS, LENS), (ROWS, LENS, empty_rows, empty_lens),
                 (empty_rows, empty_lens, empty_rows, empty_lens)):
        none = ga.query_host(*args, 0.0)
        assert none.dtype == ga.PAIR_DTYPE and none.shape == (0,)

    refused(INVALID, "gg_query_best_host: pair index out of range", ga.query_best_host, 1, 1, [(0, 2)], [a])
    refused(INVALID, "gg_query_best_host: two candidates of one rank", ga.query_best_host, 2, 1, [(0, 2)], [a], [0, 0])
    with pytest.raises(ValueError, match="^one rank per row$"):
        ga.query_best_host(2, 1, [(0, 2)], [a], [0])
    best, best_ani = ga.query_best_host(1, 2, hits, [a])
    assert best.dtype == ga.PAIR_DTYPE and best_ani.dtype == np.float32 and best.shape == best_ani.shape == (2,)
    assert best[0].tolist() == (0, 1, c, t) and best_ani[0] == a and best[1]["i"] == 0xFFFFFFFF
    best, best_ani = ga.query_best_host(0, 0, [], [])
    assert (best.dtype, best.shape, best_ani.dtype, best_ani.shape) == (ga.PAIR_DTYPE, (0,), np.float32, (0,))
    best, best_ani = ga.query_best_host(1, 1, [], [], rank=[0])
    assert best.shape == (1,) and best[0]["i"] == 0xFFFFFFFF


def test_validate_clusters_host():
    refused(INVALID, "gg_validate_clusters_host: ani is NaN", ga.validate_clusters_host, ROWS, LENS, [[0, 1]], NAN)
    refused(INVALID, "gg_validate_clusters_host: genome index out of range", ga.validate_clusters_host, ROWS, LENS,
            [[0, 2]], 0.9)
    c, t, a = expected_pair(ROWS, LENS, 0, 1)
    v = ga.validate_clusters_host(ROWS, LENS, [[0, 1]], 1.0)  # (a < 1.0: the member is too far)
    assert type(v) is ga.Validation and not v.ok
    assert (v.member_pairs, v.member_bad, v.rep_pairs, v.rep_bad) == (1, 1, 0, 0)
    assert v.bad.dtype == ga.PAIR_DTYPE and v.bad_ani.dtype == np.float32
    assert v.bad.tolist() == [(0, 1, c, t)] and v.bad_ani.tolist() == [a]
    assert v.member_violations[0].tolist() == [(0, 1, c, t)] and len(v.rep_violations[0]) == 0
    v = ga.validate_clusters_host(ROWS, LENS, [], 0.9)  # no cluster
    assert v.ok and (v.member_pairs, v.rep_pairs) == (0, 0)
    assert (v.bad.dtype, v.bad.shape, v.bad_ani.dtype, v.bad_ani.shape) == (ga.PAIR_DTYPE, (0,), np.float32, (0,))


@pytest.fixture
def fasta(tmp_path):
    rng = np.random.default_rng(3)
    path = str(tmp_path / "g.fna")
    with open(path, "wb") as f:
        f.write(b">a\n" + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100)].tobytes() + b"\n>b\nACGTNACGT\n")
    return path, str(tmp_path / "missing.fna")


def test_pack_files_and_genome_stats(fasta):
    path, missing = fasta
    refused(IO, "could not open " + missing, ga.pack_files, [path, missing])
    refused(INVALID, "gg_pack_files: invalid argument", ga.pack_files, [path], k=33)
    pk = ga.pack_files([path])
    assert type(pk) is ga.Packed and pk.n_genomes == 1 and pk.genome_kmers.shape == (1,)
    assert pk.words.dtype == np.uint32 and pk.runs.dtype == ga.RUN_DTYPE and pk.genome_kmers.dtype == np.uint64
    pk.free()
    pk = ga.pack_files([])
    assert pk.n_genomes == 0 and pk.words.shape == pk.runs.shape == pk.genome_kmers.shape == (0,)

    refused(IO, "could not open " + missing, ga.genome_stats, [path, missing])
    stats = ga.genome_stats([path])
    assert stats == [ga.GenomeAssemblyStats(2, 1, 100)]  # (contigs of 100 and 9 bases, one N)
    assert ga.calculate_genome_stats(path) == stats[0]
    assert ga.genome_stats([]) == []


def test_sketch_cache(fasta, tmp_path):
    path, _ = fasta
    cache = str(tmp_path / "cache")
    refused(INVALID, "gg_sketch_cache_load: invalid argument", ga.sketch_cache_load, cache, path, k=0)
    refused(INVALID, "gg_sketch_cache_store: invalid argument", ga.sketch_cache_store, cache, path, [1, 2, 3], s=2)
    refused(INVALID, "gg_sketch_cache_store: hashes must be strictly ascending", ga.sketch_cache_store, cache, path,
            [1, 3, 3], s=4)
    assert ga.sketch_cache_load(cache, path, s=4) is None
    assert ga.sketch_cache_store(cache, path, [1, 3, 5], s=4) is None
    got = ga.sketch_cache_load(cache, path, s=4)
    assert got.dtype == np.uint64 and got.tolist() == [1, 3, 5]


def test_parse_percentage():
    """Its own class and text: ValueError, the reference's message, no status suffix."""
    for bad, shown in ((101.0, "101"), (-1.0, "-1")):
        with pytest.raises(ValueError) as e:
            ga.parse_percentage(bad)
        assert type(e.value) is ValueError and not hasattr(e.value, "status")
        assert str(e.value) == "Invalid percentage specified for --precluster-ani: '%s'" % shown
    got = ga.parse_percentage(95)
    assert type(got) is np.float32 and got == np.float32(95.0) / np.float32(100.0)
    assert ga.parse_percentage(0.5) == np.float32(0.5) and ga.parse_percentage(1) == np.float32(0.01)


def test_update_checks_in_order():
    """FinchPreclusterer.update before it reaches a device: the paths are converted first (TypeError), then the
    state is compared (ValueError), then a path already present or given twice is refused (ValueError)."""
    state = ga.PreclusterState(["a.fna"], np.zeros((1, 8), np.uint64), [0], np.zeros(0, ga.PAIR_DTYPE), [], 21, 8, 0, 0.9)
    other = ga.FinchPreclusterer(0.9, num_kmers=4)
    with pytest.raises(TypeError):
        other.update(state, [3])
    with pytest.raises(ValueError) as e:
        other.update(state, ["a.fna"])
    assert str(e.value) == ("PreclusterState of k=21 s=8 seed=0 min_ani=%r, preclusterer of k=21 s=4 seed=0 min_ani=%r"
                            % (state.min_ani, other.min_ani))
    same = ga.FinchPreclusterer(0.9, num_kmers=8)
    for new in (["a.fna"], ["b.fna", "b.fna"]):
        with pytest.raises(ValueError) as e:
            same.update(state, new)
        assert str(e.value) == "genome already present: " + new[0]
