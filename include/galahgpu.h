/*
 * galahgpu.h -- C ABI of libgalahgpu.so, the MI355X implementation of
 * galah's finch MinHash precluster path.
 *
 * Reference interface this replaces (file:line in AroneyS/galah @ 2024-12-18):
 *
 *   src/lib.rs:23-27          trait PreclusterDistanceFinder { distances(); method_name(); }
 *   src/finch.rs:11-24        impl PreclusterDistanceFinder for FinchPreclusterer
 *   src/finch.rs:26-75        finch::distances(paths, min_ani, num_kmers, kmer_length)
 *                             -> SortedPairGenomeDistanceCache
 *     :33-47                  finch::sketch_files (needletail parse, normalize,
 *                             canonical k-mers, murmur3, bottom-s)   -> gg_pack_* + gg_sketch*
 *     :53-73                  serial all-pairs finch::distance::distance,
 *                             ani >= min_ani as f64, insert Some(ani as f32)
 *                                                                   -> gg_pairs*
 *   src/sorted_pair_genome_distance_cache.rs:22-28   key (min,max) normalisation:
 *                             every gg_pair has i < j.
 *
 * Conventions
 *   - Every entry point returns a status code; nothing throws or aborts
 *     across the ABI.  gg_last_error(ctx) (or gg_thread_last_error() for the
 *     ctx-free host functions) describes the last failure.
 *   - Inputs are borrowed for the duration of the call.  Buffers returned
 *     through pointer-to-pointer arguments are library-owned and released
 *     with gg_free / gg_packed_free.
 *   - A context drives one HIP device (gg_create) or several
 *     (gg_create_multi: one host thread per device inside each call; sketches
 *     are replicated between the devices by peer copies over xGMI and the
 *     pair tiles are partitioned).  Calls on one context must be serialised
 *     by the caller (galah calls distances() once, from one thread:
 *     src/clusterer.rs:36).
 *   - There is NO CPU fallback: gg_create fails with GG_ERR_NO_DEVICE when
 *     no MI355X (gfx950) device is visible.
 *   - *_device entry points take device pointers on the context's device
 *     and enqueue on the given hipStream_t (passed as void*; NULL is the
 *     default stream, as in HIP); they do not synchronise unless stated.
 *     When the caller shares the process with PyTorch, torch's bundled
 *     libamdhip64 must be the one loaded (import torch first) so that
 *     streams and device pointers belong to one HIP runtime.
 */
#ifndef GALAHGPU_H
#define GALAHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_ABI_VERSION 7u

typedef enum gg_status {
  GG_OK = 0,
  GG_ERR_INVALID_ARG = 1,
  GG_ERR_IO = 2,          /* file could not be opened / read */
  GG_ERR_FORMAT = 3,      /* not FASTA/FASTQ */
  GG_ERR_NO_DEVICE = 4,   /* no usable HIP device */
  GG_ERR_HIP = 5,         /* HIP runtime error */
  GG_ERR_OUT_OF_MEMORY = 6,
  GG_ERR_INTERNAL = 7,
  GG_ERR_OUTPUT_FULL = 8, /* device pair buffer too small; *count holds the need */
  GG_ERR_CANCELLED = 9    /* a caller's callback asked to stop (gg_precluster_files_each) */
} gg_status;

typedef struct gg_ctx gg_ctx;

/* One maximal stretch of A/C/G/T (after needletail normalize) inside one
 * FASTA record, at least k bases long.  Bases [base, base+len) of the
 * packed stream.  Runs of one genome are contiguous and genomes appear in
 * input order. */
typedef struct gg_run {
  uint32_t genome;
  uint32_t len;
  uint64_t base;
} gg_run;

/* One above-threshold genome pair; i < j (SortedPairGenomeDistanceCache key). */
typedef struct gg_pair {
  uint32_t i;
  uint32_t j;
  uint32_t common; /* finch raw_distance common  = |A n B|                         */
  uint32_t total;  /* finch raw_distance total   = i + j - common at first exhaustion */
} gg_pair;

/* 2-bit packed genomes: A=0 C=1 G=2 T=3, 16 bases per uint32 word, the
 * first base of a word in bits 31..30. */
typedef struct gg_packed {
  uint32_t* words;
  uint64_t n_words;
  uint64_t n_bases;
  gg_run* runs;
  uint64_t n_runs;
  uint32_t n_genomes;
  uint64_t* genome_kmers; /* per genome: number of k-mer positions (sum of len-k+1) */
} gg_packed;

/* ---- versioning / errors --------------------------------------------- */
uint32_t gg_abi_version(void);
const char* gg_status_string(gg_status s);
const char* gg_last_error(const gg_ctx* ctx);
const char* gg_thread_last_error(void);

/* ---- context ---------------------------------------------------------- */
/* kmer_length: 1..32 (galah: 21, CAP:981); sketch_size: 1..12000 (galah:
 * 1000, CAP:980); hash_seed: murmur3 seed (galah: 0, src/finch.rs:38);
 * device: HIP ordinal, or -1 for the current device. */
gg_ctx* gg_create(int kmer_length, uint32_t sketch_size, uint64_t hash_seed,
                  int device, gg_status* status);
void gg_destroy(gg_ctx* ctx);
/* HIP ordinal of the context's (first) device. */
int gg_device(const gg_ctx* ctx);

/* ---- multi-device context (SURVEY.md 8(b) n_gpus, 8(e)) ----------------- */
/* devices[0 .. n_devices): HIP ordinals, one shard each; an ordinal may
 * repeat (each entry is then its own shard with its own stream on that
 * device -- how the sharded path is exercised on one GPU).
 * devices == NULL: the first n_devices visible devices, or, for
 * n_devices == 0, the GALAHGPU_DEVICES environment variable (comma-separated
 * ordinals) when it is set and every visible device otherwise -- galah's
 * `n_gpus = 0` ("all").  One resolved device gives a plain single-device
 * context.  gg_sketch, gg_pairs, gg_sketch_files(_stats), gg_precluster_files(_cached)
 * and gg_precluster_shards use every member; the other entry points act on
 * the first member.  Results never depend on the device list. */
gg_ctx* gg_create_multi(int kmer_length, uint32_t sketch_size, uint64_t hash_seed,
                        const int* devices, uint32_t n_devices, gg_status* status);
/* Number of members (1 for a single-device context). */
uint32_t gg_device_count(const gg_ctx* ctx);
/* Member `index` as a single-device context (owned by ctx, valid until
 * gg_destroy(ctx)); ctx itself when it is a single-device context and
 * index == 0; NULL otherwise. */
gg_ctx* gg_device_ctx(gg_ctx* ctx, uint32_t index);
/* Host threads that read, gunzip and pack genome files inside
 * gg_sketch_files / gg_precluster_files(_cached): galah's --threads
 * (CAP:1327-1332).  <= 0 restores the default (GALAHGPU_THREADS, else
 * OMP_NUM_THREADS, else the CPUs of the process's affinity mask). */
gg_status gg_set_host_threads(gg_ctx* ctx, int n_threads);

/* Wall-clock phases of the last gg_precluster_files(_cached) /
 * gg_precluster_shards call on ctx, in ms: ingest + K1 (files are streamed,
 * so reading and sketching overlap), replication of the sketches between
 * devices, K2 on every device + D2H, host merge (sort by (i, j) + ANI). */
enum { GG_PHASE_SKETCH = 0, GG_PHASE_REPLICATE = 1, GG_PHASE_PAIRS = 2, GG_PHASE_MERGE = 3, GG_PHASE_COUNT = 4 };
gg_status gg_phase_times(const gg_ctx* ctx, double* ms /* [GG_PHASE_COUNT] */);

/* ---- host-side ingest: FASTA/FASTQ (plain or gz) -> 2-bit runs --------- */
/* Replaces needletail parse_fastx_file + normalize(false) + the ACGT
 * window test of canonical_kmers inside finch::sketch_files
 * (src/finch.rs:47).  Files are read on n_threads threads (<= 0: the
 * GALAHGPU_THREADS or OMP_NUM_THREADS environment variable, else the CPUs
 * in the process's affinity mask); gzip is decoded with libdeflate when the
 * system library is present, zlib otherwise. */
gg_status gg_pack_files(const char* const* paths, uint32_t n_paths,
                        int kmer_length, int n_threads, gg_packed** out);
/* In-memory records: record r (bytes seqs[r][0..lens[r]) , no header, may
 * contain line breaks) belongs to genome genome_of_record[r]; records must
 * be grouped by non-decreasing genome index. */
gg_status gg_pack_records(const uint8_t* const* seqs, const uint64_t* lens,
                          const uint32_t* genome_of_record, uint64_t n_records,
                          uint32_t n_genomes, int kmer_length, gg_packed** out);
void gg_packed_free(gg_packed* p);

/* ---- sketching (kernel K1) -------------------------------------------- */
/* Bottom-s distinct murmur3 h1 of canonical k-mers per genome, ascending;
 * bit-exact with finch's MashSketcher + process_post_filter.  out_hashes
 * is n_genomes * sketch_size (row g padded after out_lens[g]). */
gg_status gg_sketch(gg_ctx* ctx, const gg_packed* packed,
                    uint64_t* out_hashes, uint32_t* out_lens);
/* Device-resident variant: d_words / d_out / d_lens are device pointers;
 * runs is host memory (copied by the library) or device memory (a table
 * on the context's device is read in place, no copy).  Synchronises stream
 * internally (retry planning reads per-genome status). */
gg_status gg_sketch_device(gg_ctx* ctx, const uint32_t* d_words,
                           uint64_t n_words, const gg_run* runs,
                           uint64_t n_runs, uint32_t n_genomes,
                           uint64_t* d_out, uint32_t* d_lens, void* stream);

/* ---- all-pairs (kernel K2) -------------------------------------------- */
/* The pair space (i < j < n) is cut into GG_PAIR_TILE x GG_PAIR_TILE tiles
 * of the upper triangle, enumerated row-major.  Multi-GPU runs partition
 * the tile range; the union of the per-range outputs is independent of
 * the partition. */
#define GG_PAIR_TILE 64u
uint64_t gg_pair_tiles(uint32_t n);
/* Tile range [*begin, *end) of part `part` of `parts`, equal pair counts. */
void gg_pair_partition(uint32_t n, uint32_t parts, uint32_t part,
                       uint64_t* begin, uint64_t* end);

/* Host buffers in and out.  *out is library-owned (gg_free), sorted by
 * (i, j).  Pass iff ani(common,total) >= (double)min_ani, ani computed as
 * src/finch.rs:56-69 does. */
gg_status gg_pairs(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens,
                   uint32_t n, float min_ani, gg_pair** out, uint64_t* n_out);
/* Device-resident: sketches [n x sketch_size] u64, lens [n] u32 with every
 * lens[i] <= sketch_size and row i ascending in its first lens[i] entries
 * (not checked on the device; gg_pairs checks the lengths of host input).
 * Appends passing pairs of tiles [tile_begin, tile_end) to d_out (unsorted),
 * *d_count (device u64) incremented by the number found; entries past
 * out_cap are dropped (caller compares *d_count with out_cap). Async. */
gg_status gg_pairs_device(gg_ctx* ctx, const uint64_t* d_sketches,
                          const uint32_t* d_lens, uint32_t n,
                          uint64_t tile_begin, uint64_t tile_end,
                          float min_ani, gg_pair* d_out, uint64_t out_cap,
                          uint64_t* d_count, void* stream);

/* ---- adding genomes to a finished run: the border -------- */
/* For rows 0 .. n-1 and n_old <= n, the border is every pair (i < j) with
 * j >= n_old that passes gg_pairs' test, so that
 *   gg_pairs(rows[0:n]) == gg_pairs(rows[0:n_old]) U gg_pairs_border(rows[0:n], n_old),
 * the two sets disjoint.  The sketch matrix stays as it is: the old rows
 * first, the new rows after them, in the caller's order; K2 evaluates only
 * the new rows, each against every row before it.  n_old == 0 gives
 * gg_pairs, n_old == n nothing, n_old > n GG_ERR_INVALID_ARG.  A multi-device
 * context acts on its first member (the border is not sharded).
 * gg_pair_paths and gg_fallbacks count a border call like any other.  Under
 * gg_set_pairs_path MATRIX or AUTO these calls take the border form of the
 * matrix product instead (gg_pairs_border_matrix, below): the same pairs. */

/* Host buffers in and out, as gg_pairs: *out library-owned (gg_free), sorted
 * by (i, j); lens[g] <= sketch_size is checked. */
gg_status gg_pairs_border(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                          uint32_t n_old, float min_ani, gg_pair** out, uint64_t* n_out);
/* Device-resident, the contract of gg_pairs_device (appends unsorted to d_out,
 * *d_count incremented by the number found, entries past out_cap dropped,
 * asynchronous on `stream`).  A caller that keeps the matrix resident
 * between updates -- a torch tensor of [capacity x sketch_size] u64 with
 * spare rows, say -- writes each batch of new sketches after the rows it
 * holds and calls this with the grown n: nothing is moved or uploaded again. */
gg_status gg_pairs_border_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t out_cap,
                                 uint64_t* d_count, void* stream);
/* On the host (n_new * n merges at most); no device, no ctx. */
gg_status gg_pairs_border_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                               uint32_t sketch_size, int kmer_length, float min_ani,
                               gg_pair** out, uint64_t* n_out);
/* A finished run carried forward by files: only new_paths are read and
 * sketched (cache_dir as gg_sketch_files, NULL: none) into new_hashes
 * [n_new x sketch_size] and new_lens [n_new]; they are placed after the old
 * rows (old_sketches [n_old x sketch_size], old_lens, as the earlier run
 * returned them) on the device, and the border comes back sorted by (i, j)
 * with its f32 ANI (gg_free both); indices are into old + new. */
gg_status gg_update_files(gg_ctx* ctx, const uint64_t* old_sketches, const uint32_t* old_lens, uint32_t n_old,
                          const char* const* new_paths, uint32_t n_new, float min_ani, const char* cache_dir,
                          uint64_t* new_hashes, uint32_t* new_lens,
                          gg_pair** pairs, float** ani, uint64_t* n_out);

/* ---- the fused FinchPreclusterer::distances body ------------------------ */
/* paths -> sorted passing pairs plus their f32 ANI (src/finch.rs:70 value).
 * Files are streamed: read, gunzipped and packed on the host threads
 * (gg_set_host_threads) while earlier batches are copied to the devices and
 * sketched; host memory stays bounded whatever the number of files. */
gg_status gg_precluster_files(gg_ctx* ctx, const char* const* paths,
                              uint32_t n_paths, float min_ani, gg_pair** pairs,
                              float** ani, uint64_t* n_out);

/* galah's debug level (src/finch.rs:65-68 logs every compared pair): the
 * same call, plus every pair i < j of the N(N-1)/2, whatever its ANI,
 * handed to sink in blocks of whole 64-genome tile rows (at most ~4M pairs
 * each, common and total set; gg_ani_f64 gives the printed distance), in
 * (i, j) order over the call, so memory stays bounded by one block.  sink
 * returns 0 to go on; anything else ends the call with GG_ERR_CANCELLED.
 * *pairs / *ani / *n_out are the pairs >= min_ani, as gg_precluster_files
 * returns them.  cache_dir as gg_precluster_files_cached (NULL: none). */
typedef int (*gg_pair_sink)(void* user, const gg_pair* pairs, uint64_t n);
gg_status gg_precluster_files_each(gg_ctx* ctx, const char* const* paths, uint32_t n_paths,
                                   float min_ani, const char* cache_dir, gg_pair_sink sink,
                                   void* user, gg_pair** pairs, float** ani, uint64_t* n_out,
                                   uint32_t* n_cached);

/* One member's shard of device-resident packed genomes for
 * gg_precluster_shards: d_words lives on that member's device, runs (host
 * memory, or device memory: read in place on that member's device) index
 * the shard's n_genomes genomes by their genome field.  The global genome
 * order is shard 0's genomes, then shard 1's, ... */
typedef struct gg_shard {
  const uint32_t* d_words;
  uint64_t n_words;
  const gg_run* runs;
  uint64_t n_runs;
  uint32_t n_genomes;
} gg_shard;
/* The fused precluster step over genomes already resident in HBM:
 * K1 on every member's shard, sketches replicated to every member (peer
 * copies), K2 over each member's share of the pair tiles (gg_pair_partition),
 * sparse results gathered and sorted by (i, j) with their f32 ANI.
 * shards has gg_device_count(ctx) entries.  Synchronous. */
gg_status gg_precluster_shards(gg_ctx* ctx, const gg_shard* shards, float min_ani, gg_pair** pairs,
                               float** ani, uint64_t* n_out);

/* ---- sketch cache --------------------------------- */
/* galah sketches every genome on every run (src/finch.rs:47); these entry
 * points keep per-genome sketches on disk so a repeated run over the same
 * files skips ingest and K1 for them.  One entry per (genome file, k) in
 * cache_dir, valid while the file's resolved path, size and mtime and the
 * hash seed are unchanged; an entry computed with sketch size S serves any
 * s <= S (bottom-s is a prefix of bottom-S).  Results are identical with and
 * without the cache.  Format: galah_amd/csrc/sketch_cache.cpp. */

/* *hit = 1 and out_hashes[0..*out_len) filled when a valid entry exists,
 * else *hit = 0 (absent, stale, other parameters or corrupt).  Host only. */
gg_status gg_sketch_cache_load(const char* cache_dir, const char* path, int kmer_length,
                               uint32_t sketch_size, uint64_t hash_seed, uint64_t* out_hashes,
                               uint32_t* out_len, int* hit);
/* Writes (atomically replaces) the entry of path; hashes strictly ascending,
 * len <= sketch_size.  Creates cache_dir when missing.  Host only. */
gg_status gg_sketch_cache_store(const char* cache_dir, const char* path, int kmer_length,
                                uint32_t sketch_size, uint64_t hash_seed, const uint64_t* hashes,
                                uint32_t len);
/* finch::sketch_files (src/finch.rs:47) for files: out_hashes is
 * n_paths * sketch_size (row padded with 0 after out_lens[g]).  cache_dir
 * may be NULL (no cache); otherwise cached genomes are read from it and
 * the rest sketched on the device and stored (a failed store does not fail
 * the call).  *n_cached (may be NULL) receives the number of cache hits. */
gg_status gg_sketch_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths,
                          const char* cache_dir, uint64_t* out_hashes, uint32_t* out_lens,
                          uint32_t* n_cached);
/* gg_precluster_files with a sketch cache directory (NULL = none). */
gg_status gg_precluster_files_cached(gg_ctx* ctx, const char* const* paths, uint32_t n_paths,
                                     float min_ani, const char* cache_dir, gg_pair** pairs,
                                     float** ani, uint64_t* n_out, uint32_t* n_cached);

/* ---- genome assembly statistics (src/genome_stats.rs) ------------------- */
/* What galah orders the genomes by before it clusters them (the default
 * quality formulas, src/cluster_argument_parsing.rs:721-811):
 * calculate_genome_stats of src/genome_stats.rs:11-51.  A record is what the
 * packer treats as one; num_contigs counts them (empty ones too); a contig's
 * length is the bytes of its sequence lines other than '\n' and '\r';
 * num_ambiguous_bases the N and n among them; n50 the reference's loop
 * (lengths ascending, the first at which the running sum reaches
 * total_bases / 2 -- not the textbook N50); total_bases the sum of the
 * lengths (the reference does not return it). */
typedef struct gg_genome_stats {
  uint64_t num_contigs;
  uint64_t num_ambiguous_bases;
  uint64_t n50;
  uint64_t total_bases;
} gg_genome_stats;

/* src/genome_stats.rs:11 for each file, on n_threads host threads (<= 0: as
 * gg_pack_files); no device, no ctx.  File errors as gg_pack_files reports
 * them (GG_ERR_IO, GG_ERR_FORMAT; the lowest failing index). */
gg_status gg_genome_stats_files(const char* const* paths, uint32_t n_paths,
                                int n_threads, gg_genome_stats* out);

/* gg_sketch_files plus the statistics of every genome, from one read of
 * each file: the host packer takes them in its record walk, the device
 * ingest paths (device gzip inflate, GALAHGPU_PARSE=device) in a pass over
 * the batch text resident on the device.  The sketch cache is never read
 * (the statistics need the bytes); with a cache_dir every sketch computed is
 * stored, so a following gg_precluster_files_cached over the same files, in
 * any order, finds them all.  Uses every member of a multi-device context;
 * results do not depend on the device list. */
gg_status gg_sketch_files_stats(gg_ctx* ctx, const char* const* paths, uint32_t n_paths,
                                const char* cache_dir, uint64_t* out_hashes,
                                uint32_t* out_lens, gg_genome_stats* out_stats);

/* ---- after distances(): preclusters -------- */
/* src/clusterer.rs:409-431 partition_sketches (single linkage over the
 * pairs the cache contains) + :45-57 (each set sorted ascending, sets
 * ordered by size descending; ties: by smallest member).  Linear in
 * n_pairs (union-find) instead of the reference's O(N^2) contains_key
 * scan.  pairs may be in any order.  Output is CSR: precluster s is
 * members[offsets[s] .. offsets[s+1]); members has n_genomes entries,
 * offsets n_genomes + 1 (caller-owned); *n_sets receives the count. */
gg_status gg_partition_preclusters(uint32_t n_genomes, const gg_pair* pairs,
                                   uint64_t n_pairs, uint32_t* members,
                                   uint32_t* offsets, uint32_t* n_sets);

/* One pair of a precluster's sub-cache: src/sorted_pair_genome_distance_cache.rs
 * :47-58 transform_ids(precluster members) keys it (i, j), i < j, by
 * position inside the precluster; src indexes the input pairs array (for
 * its ANI value). */
typedef struct gg_local_pair {
  uint32_t precluster;
  uint32_t i;
  uint32_t j;
  uint32_t src;
} gg_local_pair;

/* transform_ids for every precluster at once (src/clusterer.rs:70), linear
 * in n_pairs instead of O(m^2) per precluster.  Every pair must lie inside
 * one precluster (true for the partition of the same pairs).  out has
 * n_pairs entries, grouped by precluster and sorted by (i, j) inside it;
 * pair_offsets has n_sets + 1 entries. */
gg_status gg_precluster_pairs(uint32_t n_genomes, const gg_pair* pairs,
                              uint64_t n_pairs, const uint32_t* members,
                              const uint32_t* offsets, uint32_t n_sets,
                              gg_local_pair* out, uint64_t* pair_offsets);

/* The two calls above as one, on the context's (first) device (DESIGN.md
 * 4.8): connected components by lock-free hooking and pointer jumping, the
 * sets and the local pairs ordered by radix sorts.  Host arrays in and out,
 * the output contract of the two host calls: members [n_genomes], offsets
 * [n_genomes + 1], *n_sets; local [n_pairs] grouped by precluster and sorted
 * by (i, j) inside it, src = index into pairs, duplicates of one pair in
 * ascending src; pair_offsets [n_genomes + 1] of which n_sets + 1 are
 * written.  local and pair_offsets may both be NULL: the partition only.
 * Pairs in any order and either orientation, duplicates allowed, i == j
 * allowed (the local pair (a, a)).  GG_ERR_INVALID_ARG for an index >=
 * n_genomes, for n_pairs or n_genomes >= 2^31 and for null arguments. */
gg_status gg_preclusters(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* pairs, uint64_t n_pairs,
                         uint32_t* members, uint32_t* offsets, uint32_t* n_sets,
                         gg_local_pair* local, uint64_t* pair_offsets);
/* Device-resident in and out on `stream`; *n_sets is a host word.
 * Synchronises the stream internally (the pointer-jumping launches go on
 * until a word read back says none of them wrote).  The input is not
 * checked: a pair with an index >= n_genomes is never followed and is left
 * out of d_local, and d_pair_offsets[n_sets] is the number of pairs written. */
gg_status gg_preclusters_device(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* d_pairs, uint64_t n_pairs,
                                uint32_t* d_members, uint32_t* d_offsets, uint32_t* n_sets,
                                gg_local_pair* d_local, uint64_t* d_pair_offsets, void* stream);

/* ---- finch + finch clustering ---------------------------- */
/* src/clusterer.rs:14-125 when the preclusterer and the clusterer are both
 * finch (skip_clusterer, :29-33, :180-185): the result is a function of the
 * pair cache alone.  n_genomes genomes in the caller's order (galah's
 * quality order: an earlier genome is preferred as representative); pairs in
 * either orientation and any order, each unordered pair at most once, only
 * their i and j are read; ani[p] the f32 the cache stores for pair p
 * (gg_ani_f32, the ani[] of gg_precluster_files); cluster_ani an f32
 * fraction, below, equal to or above the precluster threshold.
 *   :155-225  genome i is a representative unless a representative j < i has
 *             a cached pair with it and ani >= cluster_ani (f32, :212);
 *   :316-406  every other genome joins the representative, lower or higher,
 *             with the largest cached ani; ties go to the smallest index.
 * rep_of[g] receives genome g's representative (rep_of[r] == r for a
 * representative).  The host-input forms return GG_ERR_INVALID_ARG for an
 * index >= n_genomes, i == j, a NaN ani, a NaN cluster_ani or
 * n_pairs >= 2^31. */

/* On the host; no device, no ctx.  Linear in the pairs. */
gg_status gg_cluster_pairs_host(uint32_t n_genomes, const gg_pair* pairs, const float* ani,
                                uint64_t n_pairs, float cluster_ani, uint32_t* rep_of);
/* The same on the context's (first) device: host arrays in, rep_of out. */
gg_status gg_cluster_pairs(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* pairs, const float* ani,
                           uint64_t n_pairs, float cluster_ani, uint32_t* rep_of);
/* Device-resident d_pairs, d_ani and d_rep_of, on the given stream.
 * Synchronises the stream internally (the representative rounds are
 * launched until a word read back says no genome is undecided).  The input
 * is not checked: a pair with an index >= n_genomes or i == j is ignored,
 * NaN never compares >=, duplicates of a pair count once each. */
gg_status gg_cluster_pairs_device(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* d_pairs,
                                  const float* d_ani, uint64_t n_pairs, float cluster_ani,
                                  uint32_t* d_rep_of, void* stream);
/* rep_of -> CSR: cluster c is members[offsets[c] .. offsets[c+1]), clusters
 * by representative ascending, the representative first, then its members
 * ascending (galah assembles its list in rayon completion order,
 * src/clusterer.rs:114-121: no output of galah depends on an order).
 * members has n_genomes entries, offsets n_genomes + 1 (caller-owned).
 * Host only.  GG_ERR_INVALID_ARG unless rep_of[rep_of[g]] == rep_of[g] < n. */
gg_status gg_clusters_from_reps(uint32_t n_genomes, const uint32_t* rep_of, uint32_t* members,
                                uint32_t* offsets, uint32_t* n_clusters);
/* gg_precluster_files_cached(min_ani, cache_dir) followed by
 * gg_cluster_pairs(cluster_ani) over its pairs; rep_of has n_paths entries.
 * pairs / ani / n_out may all be NULL (the pairs are then freed), else they
 * receive what gg_precluster_files_cached returns. */
gg_status gg_cluster_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, float min_ani,
                           float cluster_ani, const char* cache_dir, uint32_t* rep_of,
                           gg_pair** pairs, float** ani, uint64_t* n_out);

/* ---- clustering from resident sketches ------------------- */
/* The chain of the device forms above with the pair list staying in device
 * memory: K2, the f32 ANI of every pair computed on the device, the
 * clustering step.  The pairs are not sorted on the way: neither the
 * clustering rules nor the partition into preclusters depend on their order
 * (DESIGN.md 4.5, 4.8).  Results equal those of the host-array entry points. */

/* d_ani[p] = gg_ani_f32(d_pairs[p].common, d_pairs[p].total, k of the context), bit for bit;
 * d_ani_f64 (may be NULL) the f64 before rounding; *n_rechecked (may be NULL) the entries the
 * host recomputed (those whose f32 the device's log could have rounded
 * otherwise: galah_amd/csrc/ani_core.hpp).  d_pairs 16-byte aligned,
 * n_pairs < 2^31.  Synchronises the stream. */
gg_status gg_ani_f32_device(gg_ctx* ctx, const gg_pair* d_pairs, uint64_t n_pairs, float* d_ani,
                            double* d_ani_f64, uint64_t* n_rechecked, void* stream);

typedef struct gg_cluster_summary {
  uint64_t n_pairs;            /* pairs >= min_ani */
  uint64_t ani_rechecked;      /* of them, f32 values the host recomputed (gg_ani_f32_device) */
  uint32_t n_preclusters;      /* connected components, singletons included */
  uint32_t largest_precluster;
  uint32_t pair_passes;        /* 1, or 2 after the capacity retry (0: fewer than 2 genomes) */
  uint32_t reserved;
} gg_cluster_summary;

/* rows resident -> rep_of resident; what gg_pairs + gg_ani_f32 + gg_cluster_pairs give, on
 * the context's (first) device.  d_sketches / d_lens as gg_pairs_device takes
 * them, d_rep_of [n] (every entry is written; n < 2: every genome its own
 * representative).  *d_pairs / *d_ani (may be NULL) receive context-owned device arrays of
 * summary->n_pairs entries, unsorted, valid until the next call on the context.  summary may
 * be NULL (the partition into preclusters is then not computed).
 * GG_ERR_INVALID_ARG for a NaN threshold, null buffers, n >= 2^31, or 2^31
 * passing pairs or more.  Synchronises the stream. */
gg_status gg_cluster_rows_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 float min_ani, float cluster_ani, uint32_t* d_rep_of,
                                 gg_cluster_summary* summary, const gg_pair** d_pairs, const float** d_ani,
                                 void* stream);

/* gg_cluster_files without the pair list on the host: the files sketched as
 * gg_precluster_files_cached does, then gg_cluster_rows_device over the rows
 * and rep_of [n_paths] copied back.  A multi-device context takes
 * gg_cluster_files' path instead (the resident call is not sharded) and
 * fills summary from the host partition, ani_rechecked and pair_passes 0:
 * rep_of and the other fields are the same either way.  summary may be NULL. */
gg_status gg_cluster_files_resident(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, float min_ani,
                                    float cluster_ani, const char* cache_dir, uint32_t* rep_of,
                                    gg_cluster_summary* summary);

/* ---- ANI of named pairs, cluster validation -------------- */
/* src/lib.rs:29-37 ClusterDistanceFinder::calculate_ani(fasta1, fasta2) for
 * a whole list at once: list[p].i and list[p].j name two rows of the sketch
 * matrix ([n x sketch_size] u64, lens[n], as gg_pairs takes them; rows
 * ascending without repeats); either orientation, any order, a pair may
 * repeat, i == j is allowed.  list[p].common and list[p].total receive
 * finch's merge counts (src/finch.rs:57; an empty row gives 0 and 0, i == j
 * the row's length twice), whatever the value -- there is no threshold --
 * and ani[p] (ani may be NULL) gg_ani_f32 of them.  The host-input forms
 * return GG_ERR_INVALID_ARG for an index >= n, lens[g] > sketch_size or
 * m >= 2^31. */

/* On the host (the merge itself); no device, no ctx. */
gg_status gg_ani_pairs_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                            int kmer_length, gg_pair* list, uint64_t m, float* ani);
/* The same on the context's (first) device: host arrays in and out, one
 * kernel launch per list. */
gg_status gg_ani_pairs(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, gg_pair* list,
                       uint64_t m, float* ani);
/* Device-resident: the integers only (gg_ani_f32 is host arithmetic), on the
 * given stream, asynchronous.  The input is not checked: an entry with an
 * index >= n is never followed and receives 0 and 0; a length above the
 * context's sketch size is read as the sketch size. */
gg_status gg_ani_pairs_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                              gg_pair* d_list, uint64_t m, void* stream);

/* src/cluster_validation.rs:7-78 validate_clusters with finch's ANI in the
 * place of FastANI.  clusters in gg_clusters_from_reps' CSR form (cluster c
 * is members[offsets[c] .. offsets[c+1]), its representative first; a genome
 * may occur more than once), ani the threshold as an f32 fraction; both
 * comparisons are f32 against f32 on gg_ani_f32 of the pair.
 *   :21-45  every listed genome other than its cluster's representative: bad
 *           iff its value to the representative < ani (the reference also
 *           compares the representative with itself; that pair is neither
 *           made nor counted);
 *   :47-77  every pair of clusters' representatives: bad iff >= ani (finch
 *           always yields a value: the "too divergent" arm never fires).
 * *bad (gg_free) holds the member violations as (representative, member),
 * sorted so, one per listing, then the representative violations as
 * (r1 < r2), sorted (r1 == r2 when one genome heads two clusters), with
 * common and total set; *bad_ani (gg_free) their f32.  sum->rep_pairs is
 * R (R - 1) / 2 for R clusters.  GG_ERR_INVALID_ARG for an index >= n,
 * lens[g] > sketch_size, a NaN ani, an empty cluster, offsets that do not
 * ascend, or 2^31 listed genomes or more. */
typedef struct gg_validation {
  uint64_t member_pairs;
  uint64_t member_bad;
  uint64_t rep_pairs;
  uint64_t rep_bad;
} gg_validation;

/* On the host: N + R (R - 1) / 2 merges; no device, no ctx. */
gg_status gg_validate_clusters_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                                    int kmer_length, const uint32_t* members, const uint32_t* offsets,
                                    uint32_t n_clusters, float ani, gg_validation* sum, gg_pair** bad,
                                    float** bad_ani, uint64_t* n_bad);
/* On the device: the members as one named list (first member of a
 * multi-device context), the representatives' rows through the all-pairs
 * path of gg_pairs at a threshold that keeps a superset, then the f32 rule. */
gg_status gg_validate_clusters(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                               const uint32_t* members, const uint32_t* offsets, uint32_t n_clusters, float ani,
                               gg_validation* sum, gg_pair** bad, float** bad_ani, uint64_t* n_bad);
/* gg_sketch_files(paths, cache_dir) followed by gg_validate_clusters over
 * its rows: members index paths. */
gg_status gg_validate_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, const uint32_t* members,
                            const uint32_t* offsets, uint32_t n_clusters, float ani, const char* cache_dir,
                            gg_validation* sum, gg_pair** bad, float** bad_ani, uint64_t* n_bad);

/* ---- dense ANI matrix of a set of rows ------------------ */
/* The finch ANI between every two genomes of a set -- the members of one
 * precluster or species, the representatives of a run -- as an [m x m]
 * matrix instead of a pair list: for a heatmap, a hierarchical clustering,
 * or to choose a threshold.  The shared-hash count of every two rows is the
 * product A A^T of the rows' 0/1 incidence matrix over the distinct hashes
 * that two or more of them hold, computed on the matrix cores (i8);
 * galah_amd/csrc/matrix_core.hpp states the rules.  No threshold, no gate:
 * every cell is exact. */
typedef struct gg_matrix_summary {
  uint64_t n_entries;      /* sketch entries of the listed rows */
  uint64_t n_columns;      /* distinct hashes held at >= 2 listed positions */
  uint64_t column_entries; /* entries that fall in a column */
  uint64_t ani_rechecked;  /* f32 values the host recomputed (rule of ani_core.hpp) */
} gg_matrix_summary;

/* rows[0..m) name rows of the sketch matrix ([n x sketch_size] u64, lens[n], as gg_pairs takes
 * them); rows == NULL: positions 0..m-1 are rows 0..m-1 (m <= n).  Any order, a row may be listed
 * more than once.  For positions a, b: common[a*m+b], total[a*m+b] are finch's merge counts of
 * rows[a], rows[b] exactly as gg_ani_pairs gives them (an empty row: 0 and 0; the same row, by
 * a == b or by a repeated index: its length twice), ani[a*m+b] = gg_ani_f32 of them, bit for bit.
 * Each of common / total / ani may be NULL.  m <= 32768.  The host-input
 * forms return GG_ERR_INVALID_ARG for an index >= n, lens[g] > sketch_size,
 * m > 32768, rows == NULL with m > n, or all three outputs NULL; m == 0 is
 * GG_OK and writes nothing.  summary may be NULL. */

/* On the host (the merge itself per unordered pair, mirrored); no device, no ctx. */
gg_status gg_ani_matrix_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                             int kmer_length, const uint32_t* rows, uint32_t m,
                             uint32_t* common, uint32_t* total, float* ani);
/* The same on the context's (first) device: host arrays in and out. */
gg_status gg_ani_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                        const uint32_t* rows, uint32_t m, uint32_t* common, uint32_t* total, float* ani,
                        gg_matrix_summary* summary);
/* Device-resident, on the given stream; synchronises the stream.  The rows
 * are not checked: an index >= n is never followed and is treated as an
 * empty row; a length above the context's sketch size is read as the sketch
 * size.  m * sketch size < 2^31. */
gg_status gg_ani_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                               const uint32_t* d_rows, uint32_t m, uint32_t* d_common, uint32_t* d_total,
                               float* d_ani, gg_matrix_summary* summary, void* stream);
/* gg_sketch_files(paths, cache_dir) followed by the device form over all rows. */
gg_status gg_ani_matrix_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, const char* cache_dir,
                              uint32_t* common, uint32_t* total, float* ani, gg_matrix_summary* summary);

/* ---- dense ANI matrices of many groups in one call ------ */
/* The matrix above for every group of a CSR at once -- the preclusters of a
 * run, as gg_preclusters returns them: group g is members[offsets[g] ..
 * offsets[g+1]), row indices in any order; a row may be listed twice in a
 * group and in several groups, a group may be empty; offsets[0] == 0 and
 * offsets ascend.  Block g is the [m_g x m_g] row-major matrix of the group's
 * rows, by the rules above, and begins at cell_offsets[g] = the sum of m_h^2
 * over h < g; there are no cells between groups and no cap on the number of
 * rows.  One call: P = offsets[n_groups] positions with P * sketch size <
 * 2^31, fewer than 2^32 cells, fewer than 2^31 64 x 64 tile pairs; else
 * GG_ERR_INVALID_ARG.  The summary's counts are summed over the groups (a
 * column is a hash held at two or more positions of one group). */

/* cell_offsets[0 .. n_groups] of the offsets, cell_offsets[n_groups] the
 * number of cells; host arithmetic, no ctx.  GG_ERR_INVALID_ARG for offsets
 * that do not begin at 0 or do not ascend and for the limits above (the
 * sketch size taken as 1). */
gg_status gg_ani_matrix_group_cells(const uint32_t* offsets, uint32_t n_groups, uint64_t* cell_offsets);
/* On the host (the merge itself per unordered pair of each group, mirrored);
 * no device, no ctx.  common / total / ani hold cell_offsets[n_groups]
 * entries, each may be NULL. */
gg_status gg_ani_matrix_groups_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                                    int kmer_length, const uint32_t* members, const uint32_t* offsets,
                                    uint32_t n_groups, uint32_t* common, uint32_t* total, float* ani);
/* The same on the context's (first) device: host arrays in and out.  The
 * host-input forms return GG_ERR_INVALID_ARG for an index >= n, lens[g] >
 * sketch_size or all three outputs NULL. */
gg_status gg_ani_matrix_groups(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                               const uint32_t* members, const uint32_t* offsets, uint32_t n_groups,
                               uint32_t* common, uint32_t* total, float* ani, gg_matrix_summary* summary);
/* Device-resident rows, members and outputs on the given stream; offsets is a
 * host array (the library shapes its launches from the sizes).  Synchronises
 * the stream.  The members are not checked: an index >= n is an empty row. */
gg_status gg_ani_matrix_groups_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                      const uint32_t* d_members, const uint32_t* offsets, uint32_t n_groups,
                                      uint32_t* d_common, uint32_t* d_total, float* d_ani,
                                      gg_matrix_summary* summary, void* stream);
/* The ANI matrix of every precluster of a file list: the files sketched as
 * gg_precluster_files_cached does, then, with the rows resident, K2 at
 * min_ani, gg_preclusters_device over the pair list in device memory and the
 * grouped matrices; only the results are copied back.  *members [n_paths],
 * *offsets and *cell_offsets [*n_groups + 1], *common / *total / *ani
 * [(*cell_offsets)[*n_groups]] are library-owned (gg_free); each of common /
 * total / ani may be NULL, not all three.  The groups are gg_preclusters':
 * largest first, members ascending.  A multi-device context sketches on every
 * member and runs the rest on its first. */
gg_status gg_precluster_matrices_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, float min_ani,
                                       const char* cache_dir, uint32_t** members, uint32_t** offsets,
                                       uint32_t* n_groups, uint64_t** cell_offsets, uint32_t** common,
                                       uint32_t** total, float** ani, gg_matrix_summary* summary);

/* ---- passing pairs from the matrix product -------------- */
/* gg_pairs' answer by the other way to common(i, j): the product A A^T of
 * the sections above with a thresholded epilogue, which emits the pairs at or
 * above min_ani instead of an [m x m] matrix.  Built for dense sets --
 * thousands of strains of one species -- where the inverted index pays g^2
 * member reads per hash shared by g rows.  There is no dense output and no
 * 32768-row cap: one call takes m rows with m * sketch size < 2^31 and fewer
 * than 2^31 64 x 64 tile pairs, else GG_ERR_INVALID_ARG before any row is
 * read (2,147,483 rows at sketch size 1000; 4,194,240 rows at 512 or less;
 * the tile pairs go to the device in as many launches as they need).  Pairs are (i < j) row indices of the sketch matrix with finch's merge
 * counts, exactly gg_pairs' records.  These kernels have no gg_timing_read
 * slot. */
enum { GG_PAIRS_PATH_DEFAULT = 0, GG_PAIRS_PATH_MATRIX = 1, GG_PAIRS_PATH_AUTO = 2 };

typedef struct gg_pairs_matrix_summary {
  uint64_t n_entries;     /* these three as gg_matrix_summary */
  uint64_t n_columns;
  uint64_t column_entries;
  uint64_t n_pairs;       /* passing pairs found (device form: may exceed out_cap) */
  uint64_t chunk_rounds;  /* tile pairs x ceil(n_columns / 512): upper bound of the product's work */
  uint64_t index_reads;   /* column_entries^2 / n_columns (0 without columns): lower bound of the
                             inverted index's member reads, sum of g^2 over the columns */
  uint32_t path;          /* GG_PAIRS_PATH_MATRIX or GG_PAIRS_PATH_DEFAULT: what produced the pairs */
  uint32_t pair_passes;   /* 1, or 2 after the capacity retry */
} gg_pairs_matrix_summary;

/* Device-resident, gg_pairs_device's output contract: the passing pairs among
 * the m listed rows (d_rows NULL: rows 0..m-1) are appended to d_out unsorted,
 * *d_count (device u64) grows by the number found, entries past out_cap are
 * dropped and nothing is written past out_cap.  Synchronises the stream: one
 * read-back before the product, as gg_ani_matrix_device (and, with a summary,
 * one of *d_count after it).  d_rows is not checked: an index >= n is an empty
 * row (emitted, when min_ani lets empty rows pass, with the index 0xFFFFFFFF;
 * all such positions count as one row), and a row listed twice gets its pairs
 * once per position, none with itself.  summary may be NULL. */
gg_status gg_pairs_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 const uint32_t* d_rows, uint32_t m, float min_ani, gg_pair* d_out,
                                 uint64_t out_cap, uint64_t* d_count, gg_pairs_matrix_summary* summary,
                                 void* stream);
/* Host arrays in; *out library-owned (gg_free), sorted by (i, j), as gg_pairs
 * gives it over the listed rows.  GG_ERR_INVALID_ARG for an index >= n, an
 * index listed twice, lens[g] > sketch_size, NaN min_ani or the limits above
 * (taken of n as well: every row is uploaded).  The first output capacity is
 * min(m (m - 1) / 2, max(2^20, 16 m)) pairs, with one retry at the exact
 * count.  A multi-device context acts on its first member. */
gg_status gg_pairs_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                          const uint32_t* rows, uint32_t m, float min_ani, gg_pair** out, uint64_t* n_out,
                          gg_pairs_matrix_summary* summary);
/* The border (gg_pairs_border's set: the pairs (i < j) of rows 0 .. n-1 with
 * j >= n_old) from the same product: the new rows take the
 * first positions (the sketch matrix is not moved), only tile pairs with a new
 * tile and cells of a new row are evaluated, and a hash shared among old rows
 * only is no column, so that old rows unrelated to every new row cost a
 * search and no product.  Limits, GG_ERR_INVALID_ARG before any row is read:
 * n_old <= n, n * sketch size < 2^31, fewer than 2^31 border tile pairs
 * (ceil(n_new / 64) tiles of new rows against all that follow them).
 * n_old == n gives nothing and launches nothing (*d_count is left as it is);
 * n_old == 0 is gg_pairs_matrix over all rows.  In the summary n_columns and
 * column_entries count the border's columns, chunk_rounds is the border tile
 * pairs x ceil(n_columns / 512), and index_reads is a lower bound of the
 * member reads of the index border kernel, in which every new entry reads the
 * members before it: (column_entries - e) + (e^2 / n_columns - e) / 2 with e
 * the column entries of the new rows (0 without columns).
 *
 * Device-resident: gg_pairs_border_device's output contract (appends unsorted
 * to d_out, *d_count grown by the number found, nothing written past out_cap);
 * synchronises the stream as gg_pairs_matrix_device does.  summary may be NULL. */
gg_status gg_pairs_border_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                        uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t out_cap,
                                        uint64_t* d_count, gg_pairs_matrix_summary* summary, void* stream);
/* Host arrays in; *out library-owned (gg_free), sorted by (i, j) on the
 * device, as gg_pairs_border gives it.  lens[g] <= sketch_size is checked.
 * The first output capacity is min(all border pairs, max(2^20, 16 n)), with
 * one retry at the exact count.  A multi-device context acts on its first
 * member. */
gg_status gg_pairs_border_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                                 uint32_t n_old, float min_ani, gg_pair** out, uint64_t* n_out,
                                 gg_pairs_matrix_summary* summary);
/* What produces the pairs inside gg_cluster_rows_device,
 * gg_cluster_files_resident, gg_precluster_matrices_files,
 * gg_precluster_files_resident and the border calls gg_pairs_border,
 * gg_pairs_border_device and gg_update_files.  DEFAULT (a new context's): K2
 * as ever.  MATRIX: the pair form over all rows, for a border call the border
 * form (GG_ERR_INVALID_ARG from those calls when the limits do not hold).
 * AUTO: the positions part of the matrix call (a border call: of the border
 * form) is run and its counts read back; the product is taken iff there is a
 * column, the limits hold and index_reads > R * chunk_rounds (R:
 * GALAHGPU_PAIRS_MATRIX_RATIO, by default 3,675, and 1,000 for a border call:
 * DESIGN.md 4.12, 4.13), else K2 exactly as DEFAULT.
 * Under MATRIX and AUTO gg_pairs_border_device synchronises its stream once
 * (the positions part's read-back); under DEFAULT it stays asynchronous.
 * AUTO pays the 64-bit sort of n * sketch size slots (about 0.9 ms per 10^7)
 * even when it then runs K2, which is why it is not the default.  The results
 * do not depend on the path.  An unknown value is GG_ERR_INVALID_ARG.  A
 * multi-device context sets its first member, which runs these calls. */
gg_status gg_set_pairs_path(gg_ctx* ctx, int path);
/* The path set (a null context: -1). */
int gg_pairs_path(const gg_ctx* ctx);
/* Calls of the above since creation that ran the default K2, the matrix by
 * request, and the matrix by AUTO's choice. */
gg_status gg_pairs_paths_taken(const gg_ctx* ctx, uint64_t* counts /* [3] */);
/* gg_precluster_files_cached with the rows resident on the (first) device:
 * the pairs by the context's path, sorted by (i, j) on the device,
 * gg_ani_f32_device over them, and only pairs and ANI copied back.  The
 * outputs equal gg_precluster_files_cached's whatever the path.  summary (may
 * be NULL) reports what ran; under DEFAULT its column counts are 0 (under AUTO
 * they are filled even when K2 ran). */
gg_status gg_precluster_files_resident(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, float min_ani,
                                       const char* cache_dir, gg_pair** pairs, float** ani, uint64_t* n_out,
                                       gg_pairs_matrix_summary* summary);

/* ---- a collection resident on the device ----------------- */
/* The sketch matrix of a set of genomes, its passing pairs at one min_ani in
 * (i, j) order and their f32 ANI, kept in device memory between calls:
 * genomes are added to it, removed from it, and it is clustered in any genome
 * order.  Only file bytes (or new rows) go up and rep_of comes down.
 *
 * Invariant after every successful call: the pair list equals
 * gg_pairs(rows[0:n], min_ani) in content and order, and ani[p] ==
 * gg_ani_f32(common, total, k) of pair p.
 *
 * A failed call leaves the collection as it was (a file that does not open
 * or parse, a row index out of range, out of memory, GG_ERR_INVALID_ARG at the
 * limits): new rows are written past n and n is raised last; a new pair list
 * is built in the other of two buffers, which are swapped last.
 *
 * Limits: the border calls' (n < 2^31 genomes, fewer than 2^31 pairs); a call
 * that would pass them is refused with GG_ERR_INVALID_ARG before anything is
 * changed.
 *
 * The handle is owned by the caller and tied to the gg_ctx it was made on
 * (destroy the collection first).  It acts on the context's first member, as
 * the border calls do; a multi-device context sketches files on every member
 * as gg_precluster_files_resident does and keeps the collection on the first
 * (a collection is not sharded).  A collection is not thread-safe, and every
 * call synchronises.  Its buffers are its own (never the context's scratch):
 * device_bytes reports them. */
typedef struct gg_collection gg_collection;
typedef struct gg_collection_info {
  uint64_t n_pairs;
  uint64_t pair_capacity;
  uint64_t device_bytes;
  uint32_t n_rows;
  uint32_t row_capacity;
  uint32_t grows;       /* reallocations since create */
  uint32_t rows_moved;  /* by the last gg_collection_remove */
} gg_collection_info;

/* An empty collection at min_ani (NaN is refused).  reserve_rows /
 * reserve_pairs size the buffers at once; beyond them the capacity grows
 * geometrically (allocate new, copy on the device, free old). */
gg_status gg_collection_create(gg_ctx* ctx, float min_ani, uint32_t reserve_rows, uint64_t reserve_pairs,
                               gg_collection** out);
void gg_collection_destroy(gg_collection* collection);
/* info and min_ani may each be NULL. */
gg_status gg_collection_stat(const gg_collection* collection, gg_collection_info* info, float* min_ani);
/* A collection from a state this library saved (gg_collection_rows and
 * gg_collection_pairs, or the arrays of the border calls).  What the host
 * forms check is checked: lens[g] <= sketch_size, i < j < n, the pairs
 * strictly ascending by (i, j), no NaN ANI.  The pairs are NOT recomputed:
 * the call trusts that they are gg_pairs(rows, min_ani) with their ANI. */
gg_status gg_collection_load(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                             const gg_pair* pairs, const float* ani, uint64_t n_pairs, float min_ani,
                             gg_collection** out);
/* Adding genomes: the new rows take the indices n .. n + n_new - 1, and
 * *n_border (may be NULL) receives the number of pairs added.  The border is
 * routed by the context's pairs path exactly as gg_pairs_border_device routes
 * it; gg_pair_paths, gg_pairs_paths_taken and gg_fallbacks count it like any
 * border call.  It is sorted on the device and merged into the list without
 * sorting the list again.  n_new == 0 is a no-op.
 * _rows: host rows (lens[g] <= sketch_size is checked).  _rows_device: device
 * rows, copied on `stream`, which the call synchronises (they must not be this
 * collection's own arrays: growth frees those).  _files: paths are
 * read and sketched as gg_sketch_files does (cache_dir and errors as there;
 * GG_ERR_IO / GG_ERR_PARSE leave the collection unchanged), the hashes never
 * visiting the host on a one-device context. */
gg_status gg_collection_add_rows(gg_collection* collection, const uint64_t* sketches, const uint32_t* lens,
                                 uint32_t n_new, uint64_t* n_border);
gg_status gg_collection_add_rows_device(gg_collection* collection, const uint64_t* d_sketches, const uint32_t* d_lens,
                                        uint32_t n_new, uint64_t* n_border, void* stream);
gg_status gg_collection_add_files(gg_collection* collection, const char* const* paths, uint32_t n_new,
                                  const char* cache_dir, uint64_t* n_border);
/* Removing genomes: rows [m] in any order, repeats allowed (each row counts
 * once); an index >= n is GG_ERR_INVALID_ARG.  The survivors keep their
 * relative order; new_index (may be NULL) [n before the call] receives each
 * row's new index, 0xFFFFFFFF for a removed row.  Removing nothing, or every
 * row, is valid.  The pairs of the survivors are the old pairs with both ends
 * kept, renumbered (no pair is evaluated); the rows are compacted in place,
 * rows before the first removed one untouched (info.rows_moved). */
gg_status gg_collection_remove(gg_collection* collection, const uint32_t* rows, uint32_t m, uint32_t* new_index);
/* What gg_cluster_pairs(n, the pairs renumbered by position in `order`, ani,
 * cluster_ani) returns: rep_of [n], positions in `order`.  order [n] maps
 * position -> row (NULL: the identity) and must be a permutation (checked on
 * the host, else GG_ERR_INVALID_ARG); a NaN threshold is refused. */
gg_status gg_collection_cluster(gg_collection* collection, const uint32_t* order, float cluster_ani, uint32_t* rep_of);
/* The pair list and its ANI, sorted by (i, j); gg_free both. */
gg_status gg_collection_pairs(gg_collection* collection, gg_pair** pairs, float** ani, uint64_t* n_out);
/* The rows: sketches [n x sketch_size], lens [n]. */
gg_status gg_collection_rows(gg_collection* collection, uint64_t* sketches, uint32_t* lens);
/* The device arrays themselves (each output may be NULL), valid until the next
 * call that changes the collection: gg_preclusters_device, gg_ani_matrix_device
 * and the like take them as they are. */
gg_status gg_collection_view(gg_collection* collection, const uint64_t** d_sketches, const uint32_t** d_lens,
                             const gg_pair** d_pairs, const float** d_ani);

/* ---- the query: hits and nearest representative ---------- */
/* Rows 0 .. n-1 against queries 0 .. nq-1 of the same k, sketch size and seed
 * that are NOT to be added: every cell (row i, query q) that passes the pair
 * test at the call's own min_ani (any f32; NaN is refused), as
 * gg_pair{ i, j = n + q, common, total } with finch's merge-to-first-exhaustion
 * values.  The host-returning forms give the pairs sorted by (i, j) and their
 * f32 ANI (the ANI function of the host arithmetic below, bit for bit), so that
 *
 *   query(rows, queries, min_ani)
 *     == [p for p in border(rows ++ queries, n_old = n, min_ani) if p.i < n]
 *
 * in content and order.  No query x query cell is evaluated.  min_ani <= 0:
 * every cell passes, an empty row against an empty query as (0, 0), ANI 0.
 * n == 0 or nq == 0: an empty result.  Limits, checked before any work with
 * GG_ERR_INVALID_ARG: n + nq < 2^31, and fewer than 2^31 passing pairs in the
 * forms that return to the host.  A multi-device context acts on its first
 * member, as the border does.  A query is not a pair-kernel call over tiles:
 * the pair-path, paths-taken and fallback counters do not count it.  Timing:
 * the table build under GG_KERNEL_PAIRS_INDEX (work: entries), the stream
 * kernel under GG_KERNEL_PAIRS (work: n x the batch's queries), the best hit
 * under GG_KERNEL_CLUSTER (work: hits).
 *
 * _host: no device, no context, n x nq merges.  _rows: host arrays (lens <=
 * sketch_size is checked).  _rows_device: device arrays, nothing is checked;
 * the pairs are appended unsorted by the device pair call's output contract
 * (entries past out_cap are dropped but counted, *d_count is added to, a NULL
 * d_out with out_cap 0 only counts); the call synchronises `stream`. */
gg_status gg_query_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint64_t* q_sketches,
                        const uint32_t* q_lens, uint32_t nq, uint32_t sketch_size, int kmer_length, float min_ani,
                        gg_pair** out, uint64_t* n_out);
gg_status gg_query_rows(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                        const uint64_t* q_sketches, const uint32_t* q_lens, uint32_t nq, float min_ani, gg_pair** pairs,
                        float** ani, uint64_t* n_out);
gg_status gg_query_rows_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                               const uint64_t* d_q_sketches, const uint32_t* d_q_lens, uint32_t nq, float min_ani,
                               gg_pair* d_out, uint64_t out_cap, uint64_t* d_count, void* stream);
/* The nearest candidate of every query from its hits (any order), their f32
 * ANI and rank [n] u32 (0xFFFFFFFF: the row is no candidate; NULL: every row
 * is one, rank = row): the candidate with the largest f32 ANI, ties to the
 * smallest rank -- galah's membership rule (src/clusterer.rs:376-399).
 * best[q] is the winning pair (i = 0xFFFFFFFF, j = n + q when no candidate
 * hit), best_ani[q] its ANI (0 then).  With the hits at a collection's min_ani
 * and rank = each representative's position in the clustering order, query q
 * appended last in that order would be a member of best[q].i iff best_ani[q]
 * >= cluster_ani (f32 against f32), else a new representative.  _host checks
 * index ranges, NaN ANI and that the candidates' ranks are distinct; _device
 * checks nothing and skips a pair with i >= n or j - n >= nq. */
gg_status gg_query_best_host(uint32_t n, uint32_t nq, const gg_pair* pairs, const float* ani, uint64_t n_pairs,
                             const uint32_t* rank, gg_pair* best, float* best_ani);
gg_status gg_query_best_device(gg_ctx* ctx, uint32_t n, uint32_t nq, const gg_pair* d_pairs, const float* d_ani,
                               uint64_t n_pairs, const uint32_t* d_rank, gg_pair* d_best, float* d_best_ani,
                               void* stream);
/* A collection queried: it is never changed (rows, pairs, ANI, n, capacities,
 * grows and the view pointers stay as they were).  _rows: host queries.
 * _files: the files are read and sketched exactly as the collection's add
 * sketches them (cache_dir, GG_ERR_IO / GG_ERR_PARSE of the lowest failing
 * index); q_hashes [nq x sketch_size] and q_lens [nq] (each may be NULL)
 * receive the sketches -- on a one-device context the hashes visit the host
 * only then.  The classify forms run at the collection's min_ani, keep the hit
 * list on the device and bring down best / best_ani [nq] only; rank [n] or
 * NULL as above (distinct candidate ranks are checked). */
gg_status gg_collection_query_rows(gg_collection* collection, const uint64_t* q_sketches, const uint32_t* q_lens,
                                   uint32_t nq, float min_ani, gg_pair** pairs, float** ani, uint64_t* n_out);
gg_status gg_collection_query_files(gg_collection* collection, const char* const* paths, uint32_t nq,
                                    const char* cache_dir, float min_ani, uint64_t* q_hashes, uint32_t* q_lens,
                                    gg_pair** pairs, float** ani, uint64_t* n_out);
gg_status gg_collection_classify_rows(gg_collection* collection, const uint64_t* q_sketches, const uint32_t* q_lens,
                                      uint32_t nq, const uint32_t* rank, gg_pair* best, float* best_ani);
gg_status gg_collection_classify_files(gg_collection* collection, const char* const* paths, uint32_t nq,
                                       const char* cache_dir, const uint32_t* rank, gg_pair* best, float* best_ani);

/* ---- host arithmetic shared with the caller ---------------------------- */
/* src/finch.rs:56-64: 1 - finch mash_distance, f64, Rust NaN semantics */
double gg_ani_f64(uint32_t common, uint32_t total, int kmer_length);
/* the value galah stores: Some(ani as f32), src/finch.rs:70 */
float gg_ani_f32(uint32_t common, uint32_t total, int kmer_length);
/* CAP:1160-1182 parse_percentage applied to --precluster-ani: values in
 * [1,100] are divided by 100 in f32, [0,1) kept; else GG_ERR_INVALID_ARG. */
gg_status gg_parse_percentage(float value, float* fraction);

void gg_free(void* p);

/* ---- per-kernel timing (benchmarks) ------------------------------------ */
/* When enabled, every kernel launch of the context is bracketed by HIP
 * events recorded on the stream it is launched on.  gg_timing_read
 * synchronises on those events and returns the summed duration, the number
 * of launches and the algorithmic work units (k-mer positions for
 * GG_KERNEL_SKETCH, genomes for GG_KERNEL_FINALIZE, evaluated pairs for
 * GG_KERNEL_PAIRS; GG_KERNEL_PAIRS_INDEX is the inverted-index pair kernel's
 * sort and run pass, whose pair pass counts under GG_KERNEL_PAIRS) since the
 * last gg_timing_enable.  The device-inflate ingest of gg_precluster_files /
 * gg_sketch_files (gzip lists) times its kernels too, every lane of every
 * member: the block-start search (work: compressed bytes of the batch), the
 * sub-span decode (tokens written), the expand and the resolve (text bytes),
 * the CRC-32 (text bytes), the three parse passes (text bytes, counted on
 * the first; gg_sketch_files_stats adds its two statistics passes to them)
 * and the PCIe upload of each staged batch (bytes).  GG_KERNEL_CLUSTER is
 * every kernel of gg_cluster_pairs(_device) (work: pairs, counted on the
 * first).  GG_KERNEL_ANI_PAIRS is the named-pair kernel of gg_ani_pairs(_device)
 * and gg_validate_clusters (work: listed pairs).  GG_KERNEL_PRECLUSTER is
 * every kernel of gg_preclusters(_device) (work: pairs, counted on the
 * first). */
enum { GG_KERNEL_SKETCH = 0, GG_KERNEL_FINALIZE = 1, GG_KERNEL_PAIRS = 2, GG_KERNEL_PAIRS_INDEX = 3,
       GG_KERNEL_INFLATE_SEARCH = 4, GG_KERNEL_INFLATE_DECODE = 5, GG_KERNEL_INFLATE_EXPAND = 6,
       GG_KERNEL_INFLATE_RESOLVE = 7, GG_KERNEL_INFLATE_CRC = 8, GG_KERNEL_PARSE = 9, GG_KERNEL_UPLOAD = 10,
       GG_KERNEL_CLUSTER = 11, GG_KERNEL_ANI_PAIRS = 12, GG_KERNEL_PRECLUSTER = 13, GG_KERNEL_COUNT = 14 };
typedef struct gg_kernel_stats {
  double ms;
  uint64_t launches;
  uint64_t work;
} gg_kernel_stats;
gg_status gg_timing_enable(gg_ctx* ctx, int on);
gg_status gg_timing_read(gg_ctx* ctx, int kernel, gg_kernel_stats* out);

/* ---- which pair kernel ran ---------------------------------------------- */
/* Counts since the context was created (all members of a multi-device
 * context summed), one per pair-kernel call over a tile range:
 * paths[0] the inverted index ran to completion, paths[1] the index was
 * abandoned for the gate kernel (a hash shared by more sketches than its run
 * limit, or a row's partners overflowing its map), paths[2] the gate kernel
 * ran (after an abandoned index too), paths[3] another form (table / merge,
 * GALAHGPU_PAIRS_KERNEL), paths[4] of the index calls in paths[0], those
 * whose index was built by the full 32-bit sort and run pass instead of the
 * bucketed build (a bucket too large for LDS, or GALAHGPU_INDEX_BUCKETS=0).
 * paths must hold GG_PATH_COUNT values. */
enum {
  GG_PATH_INDEX = 0,
  GG_PATH_INDEX_ABANDONED = 1,
  GG_PATH_GATE = 2,
  GG_PATH_OTHER = 3,
  GG_PATH_INDEX_FULL_SORT = 4,
  GG_PATH_COUNT = 5
};
gg_status gg_pair_paths(const gg_ctx* ctx, uint64_t* paths);

/* ---- fallbacks, peer links and one log line ---------------------------- */
/* None of these changes a result; each costs time, and galah would not see
 * it otherwise.  Counts since the context was created, members summed:
 *   GG_FALLBACK_INDEX_TO_GATE    K2 calls whose inverted index was abandoned
 *                                for the gate kernel (gg_pair_paths[1])
 *   GG_FALLBACK_INDEX_FULL_SORT  index calls rebuilt with the full 32-bit
 *                                sort after a bucket overflowed (gg_pair_paths[4])
 *   GG_FALLBACK_PEER_STAGED      sketch-row copies between two members on
 *                                different devices WITHOUT direct peer access
 *                                (the HIP runtime stages them through host
 *                                memory; see gg_peer_links)
 *   GG_FALLBACK_SKETCH_RETRY     K1 passes re-run for genomes whose first
 *                                bottom-s threshold missed (exact either way)
 *   GG_FALLBACK_INFLATE_HOST     file batches the device gzip inflate
 *                                (GALAHGPU_INFLATE=device) handed back to the
 *                                host threads (several members per file,
 *                                FASTQ, a stream it could not chain, a CRC
 *                                mismatch)
 *   GG_FALLBACK_SKETCH_SET       genomes whose candidate list outgrew its
 *                                region and were re-run in set mode (one
 *                                insert per distinct candidate; a subset of
 *                                the passes GG_FALLBACK_SKETCH_RETRY counts) */
enum {
  GG_FALLBACK_INDEX_TO_GATE = 0,
  GG_FALLBACK_INDEX_FULL_SORT = 1,
  GG_FALLBACK_PEER_STAGED = 2,
  GG_FALLBACK_SKETCH_RETRY = 3,
  GG_FALLBACK_INFLATE_HOST = 4,
  GG_FALLBACK_SKETCH_SET = 5,
  GG_FALLBACK_COUNT = 6
};
gg_status gg_fallbacks(const gg_ctx* ctx, uint64_t* counts /* [GG_FALLBACK_COUNT] */);
/* links[a * M + b] (M = gg_device_count) for members a and b: 1 when member
 * a's copies from member b go device to device (same device, or xGMI peer
 * access enabled at gg_create_multi), 0 when they are staged through host
 * memory.  A single-device context reports {1}. */
gg_status gg_peer_links(const gg_ctx* ctx, int* links /* [M * M] */);
/* One human-readable line for galah's info! log after distances(): device
 * count and ordinals, the last fused call's phase times, and the fallback
 * counts.  Writes at most cap bytes including the terminating NUL (the line
 * is cut to fit).  Returns GG_ERR_INVALID_ARG for a null ctx or buf. */
gg_status gg_info_line(const gg_ctx* ctx, char* buf, size_t cap);

/* ---- benchmark support: synthetic clustered genomes on device ---------- */
/* Genomes [first_genome, first_genome + n_genomes) of a synthetic set of
 * genomes of genome_len bases, in clusters of cluster_size consecutive
 * genomes (global index).  Member m of a cluster is the cluster root with
 * i.i.d. substitutions at rate r_m ~ U(0, max_sub_rate) (r = 0 for the
 * root itself).  Counter-based RNG: output depends only on the arguments.
 * Writes packed words (local genome g at base g*genome_len, genome_len a
 * multiple of 16) and fills runs[g] = {g, genome_len, g*genome_len} (host
 * array, local indices). */
gg_status gg_synth_clustered_device(gg_ctx* ctx, uint32_t first_genome, uint32_t n_genomes,
                                    uint32_t genome_len, uint32_t cluster_size,
                                    float max_sub_rate, uint64_t seed,
                                    uint32_t* d_words, gg_run* runs,
                                    void* stream);

/* Config C5: mixed genome lengths and N runs.  Host side,
 * deterministic in the arguments: lens[g] for genomes [first_genome,
 * first_genome + n_genomes) -- log-uniform in [min_len, max_len], rounded
 * down to a multiple of 16, shared by the members of a cluster. */
gg_status gg_synth_mixed_lengths(uint32_t first_genome, uint32_t n_genomes, uint32_t min_len,
                                 uint32_t max_len, uint32_t cluster_size, uint64_t seed,
                                 uint32_t* lens);
/* Writes the genomes (local genome g at word offset sum(lens[<g])/16) and
 * the ACGT runs between N runs: an N run starts at a base with probability
 * n_run_rate and is 1-64 bases long (those bases are excluded from every
 * run, as needletail's non-ACGT bytes break k-mers); runs shorter than k are
 * dropped.  runs has room for runs_cap entries; *n_runs receives the count
 * (GG_ERR_OUTPUT_FULL when it exceeds runs_cap). */
gg_status gg_synth_mixed_device(gg_ctx* ctx, uint32_t first_genome, uint32_t n_genomes,
                                const uint32_t* lens, uint32_t cluster_size, float max_sub_rate,
                                double n_run_rate, uint64_t seed, uint32_t* d_words, gg_run* runs,
                                uint64_t runs_cap, uint64_t* n_runs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GALAHGPU_H */
