/* ani_abi.h — C-ABI of the MI355X-native ANI engine (libfastani_amd.so).
 *
 * FastANI has no FFI/plugin interface; its seams are three C++ constructors/functions that
 * core_genome_identity() calls (all paths relative to /root/reference):
 *
 *   skch::Sketch::Sketch(const Parameters&)                         src/map/include/winSketch.hpp:109
 *   skch::Map::Map(param, sketch, totalQueryFragments&, queryno, callback)   src/map/include/computeMap.hpp:93
 *   cgi::computeCGI(param, mapResults, mapper, sketch, totalQueryFragments, queryFileNo, fileName, out)
 *                                                                   src/cgi/include/computeCoreIdentity.hpp:166
 *
 * Each entry point below replaces one of those seams (cited per function).  Plain pointers and sizes only;
 * no C++ or torch types cross this boundary.  The library is implemented with hand-written HIP kernels for
 * gfx950; there is no CPU fallback behind this ABI — every call fails with ANI_ERR_DEVICE if no GPU is usable.
 *
 * Conventions
 *   - every function returns 0 (ANI_OK) or a negative ani_status; ani_last_error() gives the message.
 *   - the caller owns all inputs; host outputs returned through `T **out` are allocated by the library and
 *     released with ani_free(); device outputs are released with ani_device_free().
 *   - one ani_ctx per device and per host thread (mirror of "one Sketch per OpenMP thread",
 *     src/cgi/core_genome_identity.cpp:55-65); a context is not thread-safe.
 *   - POD records are bit-identical to the reference structs (little-endian, 32-bit fields).
 */
#ifndef ANI_ABI_H
#define ANI_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ANI_OK = 0,
  ANI_ERR_ARG = -1,       /* invalid argument */
  ANI_ERR_DEVICE = -2,    /* no usable GPU / HIP runtime error */
  ANI_ERR_NOMEM = -3,     /* host or device allocation failed */
  ANI_ERR_LIMIT = -4,     /* input exceeds a documented limit (e.g. contig >= 2^31 bases, base_types.hpp:15) */
  ANI_ERR_INTERNAL = -5
} ani_status;

/* skch::MinimizerInfo — src/map/include/base_types.hpp:22-53 (12 bytes) */
typedef struct { uint32_t hash; int32_t seqId; int32_t wpos; } ani_minimizer_t;

/* skch::MappingResult — src/map/include/base_types.hpp:89-102 (44 bytes) */
typedef struct {
  int32_t queryLen, refStartPos, refEndPos, queryStartPos, queryEndPos, refSeqId, querySeqId;
  float nucIdentity, nucIdentityUpperBound;
  int32_t sketchSize, conservedSketches;
} ani_mapping_t;

/* cgi::CGI_Results — src/cgi/include/cgid_types.hpp:68-80 (20 bytes) */
typedef struct { int32_t refGenomeId, qryGenomeId, countSeq, totalQueryFragments; float identity; } ani_cgi_t;

/* The subset of skch::Parameters (src/map/include/map_parameters.hpp:22-41) that the hot path reads.
 * ani_params_default() fills the reference's defaults (src/map/include/parseCmdArgs.hpp:118-130) and
 * derives windowSize the way the CLI does (parseCmdArgs.hpp:225-228 -> Stat::recommendedWindowSize,
 * src/map/include/map_stats.hpp:226-256). */
typedef struct {
  int32_t kmerSize;            /* 1..16 */
  int32_t windowSize;          /* derived; 24 for k=16, fragLen=3000 */
  int32_t fragLen;             /* Parameters::minReadLength */
  float percentageIdentity;    /* 80 */
} ani_params_t;

/* A batch of genomes handed to the library.  Genome g owns contigs [genomeContigStart[g], genomeContigStart[g+1]);
 * contig c has contigLen[c] bases.
 *   layout ANI_SEQ_HOST_ASCII   : `data` is host memory, raw sequence bytes as read from FASTA (newlines removed);
 *                                 contig c starts at byte contigOffset[c].  The library upper-cases a-z
 *                                 (src/map/include/commonFunc.hpp:56-66) and leaves every other byte as is.
 *   layout ANI_SEQ_DEVICE_PACKED2: `data` is DEVICE memory, 2-bit codes A=0 C=1 G=2 T=3, 16 bases per little-endian
 *                                 uint32 (base j of a word in bits 2j..2j+1); contig c starts at WORD contigOffset[c]
 *                                 (contigs are word-aligned).  Only valid for pure-ACGT data.
 *   layout ANI_SEQ_HOST_ASCII_PTRS: as HOST_ASCII, but `data` is an array of nContigs host pointers (const uint8_t *const *), one
 *                                 per contig; contigOffset is ignored.  Lets a reader hand over per-file buffers without
 *                                 concatenating them.
 *   layout ANI_SEQ_DEVICE_BATCH   : `data` is an ani_dev_batch* returned by ani_batch_upload (genomes already packed and
 *                                 resident on the device); the table fields must describe that batch (nGenomes, nContigs,
 *                                 genomeContigStart, contigLen), contigOffset is ignored.
 *   layout ANI_SEQ_HOST_MIXED_PTRS: `data` is an array of nContigs host pointers; contigOffset[c] says what pointer c is:
 *                                 0 = raw sequence bytes (as HOST_ASCII_PTRS), 1 = 2-bit codes made by ani_pack_acgt from a
 *                                 pure-ACGT contig ((len + 15) / 16 + 2 words).  A reader packs every contig it can on its own
 *                                 thread, while the bytes are in its cache, and the upload only copies (round 6: the packing
 *                                 of a slice by the upload thread's pool was the longest stage of the command line's ingest).
 */
typedef enum { ANI_SEQ_HOST_ASCII = 0, ANI_SEQ_DEVICE_PACKED2 = 1, ANI_SEQ_HOST_ASCII_PTRS = 2, ANI_SEQ_DEVICE_BATCH = 3, ANI_SEQ_HOST_MIXED_PTRS = 4 } ani_seq_layout;
typedef struct {
  int32_t layout;
  int32_t nGenomes;
  int32_t nContigs;
  const int32_t *genomeContigStart;   /* [nGenomes+1] host */
  const int64_t *contigOffset;        /* [nContigs]   host; bytes (ASCII) or words (PACKED2) */
  const int32_t *contigLen;           /* [nContigs]   host; bases */
  const void *data;
} ani_seq_batch_t;

typedef struct ani_ctx ani_ctx;
typedef struct ani_sketch ani_sketch;
typedef struct ani_dev_batch ani_dev_batch;
typedef struct ani_fragset ani_fragset;

/* Run-time counters for the measurement contract: the algorithmic-byte figure of a run is
 * computed from these, never estimated. */
typedef struct {
  uint64_t refBases, refMinimizers, refUniqueHashes;
  uint64_t queryGenomes, queryFragments, queryBases, querySketchHashes;   /* Σ s over fragments */
  uint64_t seedHits;          /* H_total */
  uint64_t l1Candidates;
  uint64_t l2WindowEntries;   /* Σ m_c over candidates */
  uint64_t l2Steps;           /* Σ super-window placements evaluated */
  uint64_t l2QueryHashes;     /* Σ s over candidates (each candidate reads its fragment sketch once) */
  uint64_t l2WindowEntriesB, l2QueryHashesB;   /* the share of the two sums above handled by the class-B simulation launches */
  uint64_t l2Launches;        /* launches of the dominant L2 kernel (ani::k_l2_sim) */
  uint64_t l2FastCandidates;  /* candidates finished by the LDS fast path */
  uint64_t l2SlowCandidates;  /* candidates routed to the general kernel (ani::k_l2) */
  uint64_t l2SlowLimit, l2SlowDup, l2SlowOverflow;   /* ... by reason: size limits / same-hash neighbour or wide gap / counter overflow */
  uint64_t mappings;
  uint64_t cgiRows;
  uint64_t indexChunks;       /* index chunks built (one per reference set unless it passes ANI_MAX_INDEX_MINIMIZERS) */
  uint64_t l1Probes;          /* sketch hashes looked up in an index: querySketchHashes x index chunks probed */
  uint64_t l2ChunkHalvings;   /* L2 chunks redone at half size because their code stream passed the 32-bit offset limit */
  uint64_t indexChunkBuilds;  /* index chunks built, rebuilds of a streamed reference set included */
  uint64_t l1BigFragments;    /* query fragments (per index chunk) whose seed hits exceeded every LDS class: batched global-memory L1 path */
  uint64_t l1MidFragments;    /* query fragments (per index chunk) with 2048 < seed hits <= 4096: LDS class M (ani::k_l1<2048, 4096>) */
  uint64_t l1TinyFragments;   /* query fragments (per index chunk) with 1..64 seed hits: one wave each (ani::k_l1_tiny) */
  double msSketch, msIndex, msFragSketch, msL1, msL2, msReduce;   /* HIP-event time per stage, accumulated */
  double msL2Kernel;          /* HIP-event time of the class-A ani::k_l2_sim launches alone (on the launch stream) */
  double msL2Ranges, msL2Codes, msL2Slow;   /* ani::k_l2_ranges, ani::k_l2_codes, ani::k_l2 */
  double msL2SimB;            /* class-B simulation launches (ani::k_l2_sim<L2Geom<319>> + its list compaction) */
  double msL1Probe, msL1Main; /* ani::k_l1_probe; ani::k_l1<0, 2048> (the small-class gather + filter + sort + candidate kernel) */
  double msL1Big;             /* the batched global-memory L1 path (gather + device sort + candidates) */
  double msL1Tiny;            /* ani::k_l1_tiny */
} ani_counters_t;

/* ---- life cycle ---- */
int ani_init(int device, ani_ctx **out);
void ani_shutdown(ani_ctx *ctx);
const char *ani_last_error(void);
void ani_free(void *hostPtr);
void ani_device_free(ani_ctx *ctx, void *devPtr);
/* copy between device buffers of this context (used by the host side to stage records into communication buffers) */
int ani_device_copy(ani_ctx *ctx, void *dst, const void *src, size_t bytes);
/* device memory of this context (released with ani_device_free) and a copy between two contexts' devices — the host side of a
 * multi-GPU run stages minimizer records with these (peer-to-peer over xGMI when the devices can access each other) */
int ani_device_alloc(ani_ctx *ctx, size_t bytes, void **out);
/* free / total memory of the context's device in bytes (the command line sizes the blocks of a reference sketch file with it;
 * no counterpart in the reference, which splits its database by hand: scripts/splitDatabase.sh) */
int ani_device_memory(ani_ctx *ctx, size_t *freeBytes, size_t *totalBytes);
/* A hint, never needed for correctness: take from the driver NOW, on the calling thread, the device memory that sketching and
 * indexing a reference set of about `nMinimizers` minimizers will ask for (~65 bytes per minimizer: 1 GiB segments for the slices'
 * records and fragment sets first, then one segment for the index build), and leave it free in the allocator.  Fresh device memory
 * costs 20 - 40 us per MB on some hosts — 0.6 s of a cold 1000-genome run sat in the index build for that reason; the command line
 * calls this on a side thread while its readers parse the first files (estimate: input bytes x 2 / (w + 1); ANI_CLI_PREWARM=0
 * switches it off).  An estimate that is off only wastes the memory until the allocator is trimmed (ani_shutdown).  No counterpart in
 * the reference. */
int ani_pool_prewarm_index(ani_ctx *ctx, uint64_t nMinimizers);
/* The device allocator of the context's device: out[0] bytes held in segments, [1] of them free, [2] handed out, [3] segments,
 * [4] hipMalloc calls so far, [5] bytes they took, [6] microseconds they took, [7] the largest free extent of the segments that serve requests >= 32 MiB.  (The end-to-end line of
 * bench.py and the command line's trace print [5] / [6]: what fresh device memory cost on the box.)  No counterpart in the reference. */
int ani_pool_stats(ani_ctx *ctx, uint64_t out[8]);
int ani_device_copy_peer(ani_ctx *dstCtx, void *dst, ani_ctx *srcCtx, const void *src, size_t bytes);
/* Ingest: classify + 2-bit pack host sequences on host threads into page-locked staging, copy them to the
 * device and keep them there.  The handle can be passed to every entry point that takes a sequence batch (layout
 * ANI_SEQ_DEVICE_BATCH), any number of times: an all-vs-all run sketches and maps the same upload. */
int ani_batch_upload(ani_ctx *ctx, const ani_seq_batch_t *genomes, ani_dev_batch **out);
/* Host-side helper of the ingest path (no device, no context): packs `len` sequence bytes to 2 bits per base (A0 C1 G2 T3, either
 * case: commonFunc.hpp:56-66 folds a-z) into out[(len + 15) / 16 + 2] if every byte is one of A C G T a c g t and returns 1;
 * returns 0 (out undefined) if any other byte occurs — such a contig stays raw bytes (the reference hashes raw upper-cased ASCII,
 * commonFunc.hpp:71-81).  For ANI_SEQ_HOST_MIXED_PTRS. */
int ani_pack_acgt(const uint8_t *seq, int32_t len, uint32_t *out);
void ani_batch_free(ani_dev_batch *b);
int ani_get_counters(ani_ctx *ctx, ani_counters_t *out);
int ani_reset_counters(ani_ctx *ctx);

/* ---- host-side scalars: skch::Stat (src/map/include/map_stats.hpp) ---- */
int ani_params_default(ani_params_t *p, int kmerSize, int fragLen);          /* parseCmdArgs.hpp:118-130,:225-228 */
int ani_recommended_window(int kmerSize, int fragLen);                       /* map_stats.hpp:226-256 */
int ani_min_hits_relaxed(int sketchSize, int kmerSize, float identity);      /* map_stats.hpp:142-167 */
int ani_identity(int shared, int sketchSize, int kmerSize, float *nucIdentity, float *upperBound); /* computeMap.hpp:375-381 */

/* ---- reference sketch: replaces skch::Sketch::Sketch (winSketch.hpp:109-115: build :124, index :181) ---- */
int ani_sketch_build(ani_ctx *ctx, const ani_params_t *p, const ani_seq_batch_t *refs, ani_sketch **out);
void ani_sketch_destroy(ani_sketch *sk);
/* position-ordered minimizerIndex (winSketch.hpp:93) copied to the host — for parity tests and staging */
int ani_sketch_export(const ani_sketch *sk, ani_minimizer_t **out, size_t *n);
/* the numbers Sketch::sanityCheck needs (winSketch.hpp:298-318): Σ occurrences, #unique hashes, Σ contig length */
int ani_sketch_stats(const ani_sketch *sk, uint64_t *nMinimizers, uint64_t *nUnique, uint64_t *totalLength,
                     int32_t *nContigs, int32_t *nGenomes);

/* A reference set whose minimizers do not fit one 32-bit index (> ANI_MAX_INDEX_MINIMIZERS, default 1.7e9 ~ 4000 bacterial
 * genomes) is held as several index chunks cut at genome borders; every entry point below works on the whole set (global
 * seqIds / genome ids), results are identical to a single index.  This is the device-side form of the
 * reference's own database split (src/cgi/include/computeCoreIdentity.hpp:457-487, scripts/splitDatabase.sh:12-26).
 * Returns the number of chunks and (optionally, up to `cap`) the first genome id of each. */
int ani_sketch_chunks(const ani_sketch *sk, int32_t *nChunks, int32_t *firstGenome, int32_t cap);

/* Reference sets larger than the device memory (BASELINE configs[4]; the reference's own answer is the database split of
 * computeCoreIdentity.hpp:457-487 / scripts/splitDatabase.sh with every query mapped against every split): when the index
 * (~32 bytes per minimizer) does not fit beside a working-set reserve — or when ANI_MAX_RESIDENT_CHUNKS says so — the sketch keeps
 * the 12-byte minimizer records and at most `maxResident` chunks' index arrays; the mapping entry points then walk the set chunk by
 * chunk (build, map every query sub-batch, drop).  Results are identical.  Reports the mode. */
int ani_sketch_residency(const ani_sketch *sk, int32_t *streaming, int32_t *maxResident, int32_t *residentNow);
/* A sketch that holds a shard or a block of a larger reference set: `base` = global id of its first genome, added to refGenomeId in the
 * CGI rows of ani_map_cgi_batch / ani_map_cgi_fragset(s) (mapping records and ani_compute_cgi keep sketch-local ids).  The reference does this
 * per thread after the fact (cgi::correctRefGenomeIds, computeCoreIdentity.hpp:480-487, for its split of :457-474). */
int ani_sketch_set_ref_id_base(ani_sketch *sk, int32_t base);

/* Multi-GPU staging: rank r sketches its share of the reference genomes into device-resident
 * 12-byte records with GLOBAL seqIds (seqIdBase = contigs before this shard), the caller all-gathers the
 * records over RCCL (torch.distributed), and every rank builds the full index from the gathered records. */
int ani_sketch_records(ani_ctx *ctx, const ani_params_t *p, const ani_seq_batch_t *refs, int32_t seqIdBase,
                       void **devRecords, size_t *n);
int ani_sketch_from_records(ani_ctx *ctx, const ani_params_t *p, const void *devRecords, size_t n,
                            const int32_t *contigLen, int32_t nContigs,
                            const int32_t *genomeContigStart, int32_t nGenomes, ani_sketch **out);

/* The same from several record buffers (what an all-gather with one slot per rank delivers): part i holds the n[i] records of
 * genomes [partGenomeStart[i], partGenomeStart[i+1]), position order, global seqIds.  No concatenation copy is made. */
int ani_sketch_from_record_parts(ani_ctx *ctx, const ani_params_t *p, int32_t nParts, const void *const *devRecords,
                                 const uint64_t *n, const int32_t *partGenomeStart,
                                 const int32_t *contigLen, int32_t nContigs,
                                 const int32_t *genomeContigStart, int32_t nGenomes, ani_sketch **out);

/* The same, but the library TAKES the record buffers OVER (they must be device memory of this context that came from
 * ani_sketch_records / ani_sketch_records_self / ani_device_alloc; the caller must not free or touch them afterwards, whatever the
 * return code).  A set that is streamed (see ani_sketch_residency) keeps them as its records — no copy, which a set near the
 * device's capacity has no room for —, a resident set releases each buffer as soon as the index chunks that need it are built.
 * (The reference's counterpart of a set this large is the database split of computeCoreIdentity.hpp:457-487.) */
int ani_sketch_adopt_record_parts(ani_ctx *ctx, const ani_params_t *p, int32_t nParts, void *const *devRecords,
                                  const uint64_t *n, const int32_t *partGenomeStart,
                                  const int32_t *contigLen, int32_t nContigs,
                                  const int32_t *genomeContigStart, int32_t nGenomes, ani_sketch **out);

/* ---- persistent sketch file: the position-ordered minimizer records + contig / genome tables + genome names,
 * sections 4096-byte aligned (mmap-able); the reference has nothing like it (every run and every thread re-sketches).  Saving
 * costs one pass over the index; loading is an mmap, one host-to-device copy of the records and the device-side index build.
 * ani_sketch_load takes a genome range [g0, g1) (g1 < 0: all), so every rank of a multi-GPU job can read its own share. */
int ani_sketch_save(const ani_sketch *sk, const char *path, const char *const *genomeNames /* [nGenomes] or NULL */);
int ani_sketch_load(ani_ctx *ctx, const char *path, int32_t g0, int32_t g1, ani_sketch **out);
/* One file from several sketches, added one after the other (their genomes are appended): how a reference set whose minimizer
 * records exceed the device memory is written block by block.  ani_sketch_save = open + add + close.  A failed or empty writer
 * removes its file at close. */
typedef struct ani_sketch_writer ani_sketch_writer;
int ani_sketch_writer_open(const char *path, ani_sketch_writer **out);
int ani_sketch_writer_add(ani_sketch_writer *w, const ani_sketch *sk, const char *const *genomeNames /* [sk's genomes] or NULL */);
int ani_sketch_writer_close(ani_sketch_writer *w);
/* gives the writer up: the partial file is removed, the handle released (also the way out after a failed add: a close after a failed
 * add fails and removes the file as well) */
void ani_sketch_writer_abort(ani_sketch_writer *w);
int ani_sketch_file_info(const char *path, ani_params_t *p, int32_t *nContigs, int32_t *nGenomes, uint64_t *nMinimizers);
/* the genome names of a sketch file, read without loading it: *names holds the file's nGenomes NUL-terminated strings one after the
 * other (a file saved without names holds empty strings; a genome beyond the table reads as empty), *bytes their total length;
 * ani_free releases *names.  (The command line checks its queries against them before it maps anything.) */
int ani_sketch_file_names(const char *path, char **names, size_t *bytes);
const char *ani_sketch_genome_name(const ani_sketch *sk, int32_t genome);
int ani_sketch_tables(const ani_sketch *sk, const int32_t **contigLen, const int32_t **genomeContigStart);

/* ---- mapping: replaces skch::Map::Map + callback (computeMap.hpp:93-102, mapQuery :112) for ONE query genome.
 * Mappings are returned in the reference's callback order (fragment, then candidate).  *totalQueryFragments is
 * set (not accumulated). */
int ani_map_query(ani_ctx *ctx, const ani_sketch *sk, const ani_seq_batch_t *query,
                  ani_mapping_t **out, size_t *n, uint64_t *totalQueryFragments);
/* fragment sketches of one query genome (computeMap.hpp:260-274): offsets[nFragments+1], concatenated sorted
 * unique hashes — for parity tests */
int ani_query_sketch(ani_ctx *ctx, const ani_params_t *p, const ani_seq_batch_t *query,
                     uint32_t **hashes, uint64_t **offsets, size_t *nFragments);

/* ---- kept fragment sketches.  Map::Map sketches every 3-kb fragment of a query genome (computeMap.hpp:252-274) each time the
 * genome is mapped, and the reference driver re-does that per reference split (core_genome_identity.cpp:81-106).  Here the
 * fragment sketches of a batch of query genomes can be built once and kept on the device:
 *   ani_fragset_build        from query genomes;
 *   ani_sketch_records_self  all-vs-all: the genomes are references AND queries — one pass over their k-mer hashes yields both
 *                            the reference minimizer records (as ani_sketch_records) and the fragment sketches;
 *   ani_map_cgi_fragset      = ani_map_cgi_batch for the genomes of a kept set (any sketch with the same parameters).
 * qryGenomeId = firstQueryId + index of the genome in the set. */
int ani_fragset_build(ani_ctx *ctx, const ani_params_t *p, const ani_seq_batch_t *queries, ani_fragset **out);
int ani_sketch_records_self(ani_ctx *ctx, const ani_params_t *p, const ani_seq_batch_t *genomes, int32_t seqIdBase,
                            void **devRecords, size_t *n, ani_fragset **frags);
int ani_map_cgi_fragset(ani_ctx *ctx, const ani_sketch *sk, const ani_fragset *frags, int32_t firstQueryId,
                        ani_cgi_t **out, size_t *m);
void ani_fragset_free(ani_fragset *frags);
/* several kept sets in one call (set i's genomes get the query ids firstQueryIds[i] + 0, 1, ...): a streamed reference set builds
 * each of its index chunks once per call, so hand over everything that is to be mapped.  Rows: set by set, (query, reference). */
int ani_map_cgi_fragsets(ani_ctx *ctx, const ani_sketch *sk, int32_t nSets, const ani_fragset *const *frags, const int32_t *firstQueryIds,
                         ani_cgi_t **out, size_t *m);
int ani_fragset_info(const ani_fragset *frags, int32_t *nGenomes, int64_t *nFragments, uint64_t *nHashes);
/* A kept set as ONE device buffer (header + tables + hash pool; plain bytes for RCCL send/recv or all-gather) and back: the
 * multi-GPU path shards the REFERENCES, every GPU indexes its shard only, and the query fragment sketches — a third of the size
 * of the minimizer records — travel between the GPUs.  ani_fragset_unpack returns a view: the arrays stay
 * in devBuf, which must outlive the set. */
int ani_fragset_pack_bytes(const ani_fragset *frags, size_t *bytes);
int ani_fragset_pack(ani_ctx *ctx, const ani_fragset *frags, void *devBuf, size_t cap, size_t *bytes);
int ani_fragset_unpack(ani_ctx *ctx, const void *devBuf, size_t bytes, ani_fragset **out);
/* ONE set over several packed sets that lie in one device buffer at a fixed pitch (slot i at devBuf + i * slotBytes) — what an
 * all-gather of the ranks' packed sets delivers.  slotQueryBase[i] = query id of slot i's first genome (ascending over the slots),
 * or < 0 to leave the slot out (the rank's own); rows come back with qryGenomeId = firstQueryId + that id.  The hash pools stay in
 * devBuf (which must outlive the set and span < 2^32 hashes); only the per-fragment tables are copied.  Mapping the merged set is one
 * pass of the kernels instead of one per set — the reference's loop has this shape too: per reference split, ALL queries
 * (core_genome_identity.cpp:55-106). */
int ani_fragset_unpack_merged(ani_ctx *ctx, const void *devBuf, size_t slotBytes, int32_t nSlots, const int32_t *slotQueryBase,
                              ani_fragset **out);

/* ---- reducer: replaces cgi::computeCGI (computeCoreIdentity.hpp:166-298) for one query genome ----
 * The mappings may come in any order (a list that is not ordered by (querySeqId, refSeqId) is sorted on the device); querySeqId values
 * need not be dense.  Rows: refGenomeId ascending, the sketch's own ids (ani_sketch_set_ref_id_base does not apply), qryGenomeId =
 * queryFileNo, totalQueryFragments as given; n = 0 gives no rows.  ANI_ERR_ARG, with nothing reduced, for a mapping with
 *   - refSeqId outside [0, contigs of the sketch),
 *   - refStartPos outside [0, length of that contig] (the length itself is accepted: it falls into the contig's last bin),
 *   - nucIdentity outside (0, 100]: zero, -0.0, negative, above 100, +inf or NaN (the reducer orders identities by their bit
 *     patterns and sums them, so a NaN would displace every valid identity of its bin and poison the row),
 *   - a negative querySeqId;
 * ANI_ERR_LIMIT for 2^31 - 16 mappings or more. */
int ani_compute_cgi(ani_ctx *ctx, const ani_sketch *sk, const ani_mapping_t *mappings, size_t n,
                    uint64_t totalQueryFragments, int32_t queryFileNo, ani_cgi_t **out, size_t *m);

/* ---- fused many-to-many path: the query loop of core_genome_identity.cpp:81-106 for a whole batch of query
 * genomes, device-resident end to end (Map + computeCGI per query; no mapping records leave the GPU).
 * Row order: query id ascending, then refGenomeId ascending.  qryGenomeId = firstQueryId + index in batch. */
int ani_map_cgi_batch(ani_ctx *ctx, const ani_sketch *sk, const ani_seq_batch_t *queries, int32_t firstQueryId,
                      ani_cgi_t **out, size_t *m);

/* ---- per-bin conservation profile of the reference genomes (no counterpart in the reference, which folds the bin table of
 * computeCoreIdentity.hpp:237-254 into a row per pair and drops it).  Between begin and end the sketch adds up,
 * per reference bin of fragLen - 20 bases, how many query genomes reached the bin and how identical they were there: the bins present
 * in every query are the core genome, the others islands.  Everything is integer or bit pattern: the result depends on no schedule,
 * reduction order, sub-batch size, index chunking, residency mode or order of calls.
 *  1. Bins.  Contig c of the sketch (set-global contig id, the order of ani_sketch_tables) has contigLen[c] / (fragLen - 20) + 1 bins;
 *     bin j holds the start positions [j (fragLen - 20), (j + 1)(fragLen - 20)).  Bins are numbered contig by contig over the whole set:
 *     binStart[c] = the bins of the contigs before c, nBins = binStart[nContigs] (64 bit; the numbering does not restart with an index
 *     chunk).
 *  2. Cell.  For a query genome q reduced against the sketch, cell(q, b) is what the reducer's bin table holds for bin b: the maximum,
 *     over the fragments f of q whose 1-way winner lies in b, of that winner's identity; the 1-way winner of f is the maximum under
 *     (nucIdentity bits, refSeqId, refStartPos) over f's mappings to b's genome; no such fragment: the cell is empty.  The row of
 *     (q, g) stays what it is: countSeq = the non-empty cells of g, identity = their float mean in bin order.
 *  3. Gate.  The pair (q, g) contributes iff it has a row, countSeq >= minFragments and bits(identity) >= bits(minIdentity);
 *     minIdentity in [0, 100] (-0.0 counts as 0), minFragments >= 1.
 *  4. Accumulation, per contributing pair: queries[g] += 1, and for every non-empty cell of g: count[b] += 1, sum[b] += fix(cell),
 *     minIdentity[b] / maxIdentity[b] by bit pattern; fix(x) = (uint64_t) llrint((double) x * 2^20), round half even (exact for
 *     x >= 8; a sum of 2^32 cells stays below 2^59).  A bin with count = 0 reads {0, 0.0f, 0.0f, 0, 0}.
 *  5. Which calls.  Every call that reduces against the sketch between begin and end: ani_map_cgi_batch, ani_map_cgi_fragset(s),
 *     ani_compute_cgi (and the test entry point ani_reduce_check); ani_map_query reduces nothing and adds nothing.  A genome mapped
 *     twice counts twice.  A call that fails before it reduces anything (the argument checks of ani_compute_cgi) leaves the profile as
 *     it was; after any other failed call the profile is unspecified until the next begin.
 *  6. Rows are untouched: with or without a profile every mapping call returns the same rows, bit for bit.
 * begin allocates and zeroes the accumulators on the device (20 bytes per bin + 4 per genome; 3 GB for 90 000 x 5 Mbp); a second begin
 * resets them and takes the new gate.  bins works with or without a begin.  read does not reset; either pointer may be NULL.  end releases
 * (ani_sketch_destroy does too).  ANI_ERR_ARG: a null sketch, minIdentity outside [0, 100] (NaN included), minFragments < 1, read or end
 * without a begin; ANI_ERR_NOMEM: the device cannot hold the accumulators (the scalar checks come first); ANI_ERR_LIMIT at read: count and
 * queries are 32 bit and a counter has reached 2^32 - 1 (it stays there instead of wrapping).  ani_sketch_save does not write the profile,
 * and ani_sketch_set_ref_id_base does not apply: bins and genomes are the sketch's own. */
typedef struct { uint32_t count; float minIdentity, maxIdentity; uint32_t reserved; uint64_t sum; } ani_binprofile_t;   /* 24 bytes */
int ani_sketch_profile_begin(ani_sketch *sk, float minIdentity, int32_t minFragments);
int ani_sketch_profile_bins(const ani_sketch *sk, uint64_t *nBins);
int ani_sketch_profile_read(const ani_sketch *sk, ani_binprofile_t *bins /* [nBins] */, uint32_t *queries /* [nGenomes] */);
int ani_sketch_profile_end(ani_sketch *sk);

/* ---- per-pair fragment identity distributions (no counterpart in the reference: an ANI value is the mean of the pair's cells, and the
 * spread behind it is dropped with the bin table).  Between begin and end every call that reduces against the
 * sketch (the calls of the profile's rule 5; ani_map_query adds nothing) appends one record per contributing pair to a list on the host,
 * which take hands over.  Everything is integer or bit pattern.
 *  1. Values.  For a pair (q, g), V is the multiset of the non-empty cells of g's bins for q (a cell: the profile's rule 2);
 *     count = |V| = the row's countSeq.
 *  2. Gate: the profile's rule 3.  The pair contributes iff it has a row, countSeq >= minFragments and bits(identity) >= bits(minIdentity);
 *     minIdentity in [0, 100] (-0.0 counts as 0), minFragments >= 1.
 *  3. Classes.  nEdges in 0 .. 63 finite floats in [0, 100], strictly ascending (-0.0 counts as 0).  class(x) = the number of edges e with
 *     edges[e] <= x: a float comparison and, for these values, one of bit patterns; no arithmetic touches x.  A record has nEdges + 1
 *     counters hist[class]; they add up to count.  A value bit-equal to an edge belongs to the class above the edge.
 *  4. Order statistics, on the bit patterns.  With V sorted ascending as v[0 .. count - 1]: minIdentity = v[0], q1 = v[(count - 1) / 4],
 *     median = v[(count - 1) / 2], q3 = v[3 (count - 1) / 4], maxIdentity = v[count - 1], the divisions integer: each of the five is a
 *     value some cell holds.
 *  5. Sum.  sum = the sum over V of fix(v), the profile's fix(x) = (uint64_t) llrint((double) x * 2^20).
 *  6. Ids and order.  qryGenomeId and refGenomeId are those of the ani_cgi_t row the same call returned for the pair (firstQueryId, the
 *     query ids of a merged set and ani_sketch_set_ref_id_base included).  The records of one call come in the order of that call's rows,
 *     restricted to the pairs that pass the gate; calls follow each other in call order.
 *  7. Rows are untouched: with the mode on or off every mapping call returns the same rows, bit for bit.  The profile and the
 *     distribution can be on together and do not see each other.
 *  8. Determinism.  Nothing depends on schedule, sub-batch size, index chunking, residency (resident, chunked, streamed) or piece sizes.
 * begin starts (a second begin drops what is pending and takes the new gate and edges).  take hands over everything appended since begin
 * or the last take and empties the list: rec[n], and, unless `hist` is NULL, hist[n][nEdges + 1]; both are released with ani_free; with
 * n = 0 both come back NULL.  A caller that drains after every mapping call holds one call's worth (40 + 4 (nEdges + 1) bytes per record
 * of host memory until taken).  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null sketch (or rec or n), a gate outside its
 * ranges (NaN included), nEdges outside 0 .. 63, null edges with nEdges > 0, an edge that is NaN, infinite, outside [0, 100] or not above
 * its predecessor, take or end without a begin; a refused begin leaves a running distribution as it was.  ANI_ERR_NOMEM: the records do
 * not fit the host.  After a call that failed while reducing, the pending list is unspecified until the next begin. */
typedef struct { int32_t refGenomeId, qryGenomeId; uint32_t count;
                 float minIdentity, q1, median, q3, maxIdentity; uint64_t sum; } ani_fragdist_t;  /* 40 bytes */
int ani_sketch_fragdist_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, const float *edges, int32_t nEdges);
int ani_sketch_fragdist_take(ani_sketch *sk, ani_fragdist_t **rec, uint32_t **hist, size_t *n);
int ani_sketch_fragdist_end(ani_sketch *sk);

/* ---- reciprocal best-hit records of the fused path (the reference prints such records for --visualize only, one query genome per call
 * and from a std::sort on the host).  Between begin and end every call that reduces against the sketch (the calls
 * of the profile's rule 5; ani_map_query adds nothing) appends one record per non-empty cell of every contributing pair to a list on the
 * host, which take hands over.  Everything is integer or bit pattern.
 *  1. 1-way winner: the profile's rule 2.  For a fragment f of query genome q and a reference genome g it is the maximum under
 *     (nucIdentity bits, refSeqId, refStartPos) over f's mappings to g; it lies in bin b = refStartPos / (fragLen - 20) of its contig.
 *  2. Cell winner.  cell(q, b) = the maximum identity over the fragments whose 1-way winner lies in b.  The cell's hit is the fragment with
 *     the LARGEST querySeqId among those whose 1-way winner lies in b with identity bits equal to the cell's.  querySeqId is unique per
 *     fragment of a genome, so the hit is unique.  A fragment whose 1-way winner loses its cell has no record for that pair, even if
 *     another of its mappings would have won a different cell.  (A stated tie rule: the reference leaves equal identities in one bin to
 *     the order std::sort happens to produce.)
 *  3. Gate: the profile's rule 3.  The pair contributes iff it has a row, countSeq >= minFragments and bits(identity) >= bits(minIdentity);
 *     minIdentity in [0, 100] (-0.0 counts as 0), minFragments >= 1.
 *  4. Record.  refGenomeId and qryGenomeId are those of the ani_cgi_t row the same call returned for the pair (firstQueryId, the query ids
 *     of a merged set and ani_sketch_set_ref_id_base included).  refSeqId is the sketch's own set-global contig id, in the order of
 *     ani_sketch_tables; the id base does not apply to it.  refStartPos and identity are those of the winning mapping, bit for bit.
 *     querySeqId is the value ani_map_query reports for that fragment; for ani_compute_cgi (and ani_reduce_check) the mapping's own
 *     querySeqId as given — not dense, up to 2^31 - 1.
 *  5. Count.  A contributing pair has exactly countSeq records; their identities, summed in float in record order and divided by the
 *     count, give the row's identity bit for bit.
 *  6. Order.  The records of one call come in the order of that call's rows, restricted to the pairs that pass the gate; within a pair in
 *     bin order, (refSeqId, bin) ascending; calls follow each other in call order.
 *  7. Rows are untouched: with the mode on or off every mapping call returns the same rows, bit for bit.  The profile, the distributions
 *     and the hits can be on together and do not see each other.
 *  8. Determinism.  Nothing depends on schedule, sub-batch size, index chunking, residency (resident, chunked, streamed) or piece sizes.
 * begin starts (a second begin drops what is pending and takes the new gate).  take hands over everything appended since begin or the
 * last take and empties the list: rec[n], released with ani_free; with n = 0 it comes back NULL.  24 bytes per record of host memory until
 * taken; the gate is the remedy for sets whose records do not fit.  While the mode is on the device holds one more uint32 per cell of a
 * sub-batch's bin table.  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null sketch (or rec or n), a gate outside its ranges
 * (NaN included), take or end without a begin; a refused begin leaves a running mode as it was.  ANI_ERR_NOMEM: the records do not fit the
 * host, or the device cannot hold the extra table.  ANI_ERR_LIMIT: more than 2^32 - 16 records in one (sub-batch, index chunk).  After a
 * call that failed while reducing, the pending list is unspecified until the next begin. */
typedef struct { int32_t refGenomeId, qryGenomeId, refSeqId, refStartPos, querySeqId; float identity; } ani_hit_t;  /* 24 bytes */
int ani_sketch_hits_begin(ani_sketch *sk, float minIdentity, int32_t minFragments);
int ani_sketch_hits_take(ani_sketch *sk, ani_hit_t **rec, size_t *n);
int ani_sketch_hits_end(ani_sketch *sk);

/* ---- percentile bootstrap intervals of the ANI values (no counterpart in the reference: an ANI value is the mean of the pair's cells,
 * and "95.1" from 1 600 cells prints like "95.1" from 40).  Between begin and end every call that reduces against
 * the sketch (the calls of the profile's rule 5; ani_map_query adds nothing) appends one record per contributing pair to a list on the
 * host, which take hands over.  Everything is integer and a stated counter-based hash.
 *  1. Values.  For a pair (q, g), v[0 .. count - 1] are the non-empty cells of g's bins for q (a cell: the profile's rule 2), taken in bin
 *     order, ascending bin number from genomeBinStart[g]; count is the row's countSeq.  F[i] = fix(v[i]), the profile's
 *     fix(x) = (uint64_t) llrint((double) x * 2^20); sum = the sum of the F[i].
 *  2. Gate: the profile's rule 3.  The pair contributes iff it has a row, countSeq >= minFragments and bits(identity) >= bits(minIdentity);
 *     minIdentity in [0, 100] (-0.0 counts as 0), minFragments >= 1.
 *  3. Draws.  fmix32 is MurmurHash3's 32-bit finalizer: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16, all
 *     arithmetic mod 2^32.  For replicate r in 0 .. B - 1 and draw j in 0 .. count - 1:
 *       k(r) = fmix32(seed + 0x9e3779b9 (r + 1)),   u(r, j) = fmix32(k(r) ^ (0x85ebca6b (j + 1))),
 *       idx(r, j) = ((uint64_t) u(r, j) * count) >> 32,   S[r] = the sum over j of F[idx(r, j)], a uint64 below 2^59.
 *     The draws depend on (seed, r, j, count) only, not on the pair: common random numbers.  Two pairs with equal count resample the same
 *     positions, so their intervals differ by their cells and not by their luck, and nothing depends on where a query sits in a sub-batch.
 *  4. Interval.  L = levelPermille in 1 .. 999, lowRank = ((B - 1)(1000 - L)) / 2000 (integer division), highRank = B - 1 - lowRank.  With
 *     S sorted ascending, lowSum = S[lowRank] and highSum = S[highRank]; low = (float)((double) lowSum / ((double) count * 1048576.0)), high
 *     likewise (computed on the host).  Neither is clamped, and neither is forced to bracket the row's identity.  A pair whose cells are all
 *     bit-equal has lowSum = highSum = sum; count = 1 is that case.
 *  5. Ids and order: the distributions' rule 6.  The ids of the row the same call returned, in the rows' order, restricted to the gated
 *     pairs; calls follow each other in call order.
 *  6. Rows are untouched.  The profile, the distributions, the hits and the intervals can all be on together and do not see each other.
 *  7. Determinism: the distributions' rule 8.  Nothing depends on schedule, sub-batch size, index chunking, residency or piece sizes.
 * begin starts (a second begin drops what is pending and takes the new gate, B, L and seed).  take hands over everything appended since
 * begin or the last take and empties the list: rec[n], released with ani_free; with n = 0 it comes back NULL.  48 bytes per record of host
 * memory until taken.  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null sketch (or rec or n), a gate outside its ranges
 * (NaN included), replicates outside 1 .. 1024, levelPermille outside 1 .. 999, take or end without a begin; a refused begin leaves a
 * running mode as it was.  ANI_ERR_NOMEM: the records do not fit the host, or the device cannot hold a piece.  After a call that failed
 * while reducing, the pending list is unspecified until the next begin. */
typedef struct { int32_t refGenomeId, qryGenomeId; uint32_t count, replicates;
                 uint64_t sum, lowSum, highSum; float low, high; } ani_ci_t;   /* 48 bytes */
int ani_sketch_ci_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, int32_t replicates /* 1..1024 */,
                        int32_t levelPermille /* 1..999 */, uint32_t seed);
int ani_sketch_ci_take(ani_sketch *sk, ani_ci_t **rec, size_t *n);
int ani_sketch_ci_end(ani_sketch *sk);

/* ---- the bootstrap replicate sums of the ANI values as records (what the intervals draw and reduce to two order statistics, kept: the
 * input of the trees' support values, ani_tree_support_bootstrap).  Between begin and end every call that reduces
 * against the sketch (the calls of the profile's rule 5; ani_map_query adds nothing) appends one record and `replicates` sums per
 * contributing pair to two lists on the host, which take hands over.  Everything is integer and the intervals' stated hash.
 *  1. Values, gate, draws: the intervals' rule 1 word for word, their rule 2 (with this mode's own minIdentity and minFragments) and their
 *     rule 3.  sums[i * B + r] is exactly the S[r] of that rule for pair i, r in 0 .. B - 1, in replicate order, not sorted; sum is the
 *     sum of the F.  A pair whose cells are all bit-equal has S[r] = sum for every r; count = 1 is that case.
 *  2. Consistency with the intervals.  With the same seed and B, the sorted S at lowRank and highRank of the intervals' rule 4 equal
 *     ani_ci_t.lowSum and highSum of the same pair, and sum equals ani_ci_t.sum.
 *  3. Replicate identity, computed by the caller and stated once: id_r = (float)((double) S[r] / ((double) count * 1048576.0)), the
 *     formula of the intervals' rule 4.
 *  4. Ids and order: the rows', as the intervals' rule 5.
 *  5. Independence.  Rows are untouched.  Every other mode can be on beside it, the intervals included; each has its own gate, B and seed.
 *  6. Determinism.  Nothing depends on schedule, sub-batch size, index chunking, residency or piece size.
 * begin starts (a second begin drops what is pending and takes the new gate, B and seed).  take hands over everything appended since
 * begin or the last take and empties the lists: rec[n] and sums[n * replicates], each released with ani_free; an empty list comes back
 * NULL with 0 (sums may be null: the sums are then dropped).  24 + 8 B bytes per record of host memory until taken; the device holds one
 * piece, at most 2^28 bytes of sums.  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null sketch (or rec or n), a gate
 * outside its ranges (NaN included), replicates outside 1 .. 1024, take or end without a begin; a refused begin leaves a running mode as
 * it was.  ANI_ERR_NOMEM: the records do not fit the host, or the device cannot hold a piece.  After a call that failed while reducing,
 * the pending lists are unspecified until the next begin. */
typedef struct { int32_t refGenomeId, qryGenomeId; uint32_t count, replicates; uint64_t sum; } ani_boot_t;   /* 24 bytes */
int ani_sketch_boot_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, int32_t replicates /* 1..1024 */, uint32_t seed);
int ani_sketch_boot_take(ani_sketch *sk, ani_boot_t **rec, uint64_t **sums /* [n][replicates] */, size_t *n);
int ani_sketch_boot_end(ani_sketch *sk);

/* ---- the best reference of every query fragment over the whole reference set ("genome painting"; no counterpart in the reference, whose
 * outputs are all per pair of genomes).  Between begin and end every call that reduces against the sketch (the
 * calls of the profile's rule 5; ani_map_query adds nothing) appends one record per mapped query fragment to a list on the host, which
 * take hands over.  The records are per fragment, not per pair, and know no gate.  Everything is integer or bit pattern.
 *  1. 1-way winner: rule 1 of the hits.  For a fragment f and a reference genome g it is the maximum under (nucIdentity bits, refSeqId,
 *     refStartPos) over f's mappings to g with identity bits != 0; a genome without such a mapping has no winner.
 *  2. Order of genomes for a fragment: the genome whose winner has the higher identity bits comes first; at equal bits the SMALLER
 *     refGenomeId, with the ids as the records carry them (the "preferred genomes first" convention of ani_cluster_greedy).
 *  3. Record.  One record per fragment that has at least one winner, none for a fragment that has none.  qryGenomeId, querySeqId: the
 *     fragment (ids as rule 4 of the hits gives them: firstQueryId, the query ids of a merged set; querySeqId as ani_map_query reports
 *     it, for ani_compute_cgi and ani_reduce_check the mapping's own — not dense, up to 2^31 - 1).  refGenomeId, refSeqId, refStartPos,
 *     identity: the first genome under rule 2 (ani_sketch_set_ref_id_base included) and its 1-way winner, bit for bit; refSeqId is the
 *     sketch's own set-global contig id.  secondGenomeId, secondIdentity: the second genome under rule 2 and the identity of its
 *     winner, -1 and 0.0f where one genome only has a winner.  genomes: the number of reference genomes with a winner.  reserved = 0.
 *  4. Order.  The records of one call follow the call's query order, then querySeqId ascending; calls follow each other in call order.
 *  5. Independence.  Nothing depends on schedule, sub-batch size, index chunking, residency (resident, chunked, streamed) or piece size.
 *     Rows are untouched; the profile, the distributions, the hits and the intervals can be on beside it and do not see it.
 *  6. Merge.  ani_paint_merge(a, na, b, nb, &out, &n): a and b are record lists over DISJOINT sets of reference genomes, each ordered by
 *     (qryGenomeId, querySeqId) ascending; out is the list over the union, in that order: a fragment in one list only is copied; for a
 *     fragment in both, genomes is the sum, first and second are the top two under rule 2 of the up to four (genome, identity) entries
 *     the two records hold, and refSeqId and refStartPos travel with the first.  out[n] is released with ani_free (n = 0: NULL).  A pure
 *     host function: no context.  The engine joins the partial records of the index chunks of a set with it (their genomes are
 *     disjoint); callers join shards, blocks and splits of a reference set, after giving the records their final ids.
 * begin starts; take hands over everything appended since begin or the last take and empties the list: rec[n], released with ani_free;
 * with n = 0 it comes back NULL.  40 bytes per record of host memory until taken, 24 bytes per fragment of a sub-batch on the device
 * while the mode is on.  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null pointer, a begin while the mode is on, take
 * or end without a begin, a list out of order (merge).  ANI_ERR_NOMEM: host or device memory.  ANI_ERR_LIMIT: more than 2^32 - 16
 * records in one (sub-batch, index chunk).  After a call that failed while reducing, the pending list is unspecified until end. */
typedef struct { int32_t qryGenomeId, querySeqId, refGenomeId, refSeqId, refStartPos; float identity;
                 int32_t secondGenomeId; float secondIdentity; uint32_t genomes, reserved; } ani_paint_t;   /* 40 bytes */
int ani_sketch_paint_begin(ani_sketch *sk);
int ani_sketch_paint_take(ani_sketch *sk, ani_paint_t **rec, size_t *n);
int ani_sketch_paint_end(ani_sketch *sk);
int ani_paint_merge(const ani_paint_t *a, size_t na, const ani_paint_t *b, size_t nb, ani_paint_t **out, size_t *n);

/* ---- collinear blocks and breakpoints of a pair's reciprocal best hits (the ORDER of the hits, which the reference shows only as the
 * dot plot of --visualize, one pair per run).  Between begin and end every call that reduces against the sketch
 * (the calls of the profile's rule 5; ani_map_query adds nothing) appends one pair record per contributing pair and one block record per
 * collinear block of it to two lists on the host, which take hands over.  Everything is integer arithmetic on the pair's best-hit records
 * as rules 1 - 6 of the hits define them: the synteny records of a pair are a pure function of that pair's hit records.
 *  1. Input.  A pair that passes the gate (the hits' rule 3, with this mode's own minIdentity and minFragments) has the hits
 *     h[0 .. n - 1] in bin order (the hits' rule 6), n = countSeq; q[i] = querySeqId, c[i] = refSeqId, p[i] = refStartPos, F[i] =
 *     fix(identity) = (uint64_t) llrint((double) identity * 2^20) of h[i].  The q[i] of one pair are distinct.
 *  2. Rank.  r[i] = the number of j with q[j] < q[i]: the rank among the pair's own hits, not the id itself.  Fragments that mapped
 *     nowhere and insertions of unmatched sequence therefore break nothing; querySeqId need not be dense and goes up to 2^31 - 1.
 *  3. Adjacency (i, i + 1), 0 <= i < n - 1, has exactly one class: `contig` if c[i] != c[i + 1]; else `forward` if r[i + 1] = r[i] + 1;
 *     else `reverse` if r[i + 1] = r[i] - 1; else `break`.  (Ranks are distinct, so forward is never directly followed by reverse.)
 *  4. Block.  A maximal run of consecutive hits joined by forward / reverse adjacencies; its direction is +1, -1, or 0 for a block of one
 *     hit (a singleton).
 *  5. Pair record.  refGenomeId and qryGenomeId as the hits' rule 4 gives them; count = n; forward, reverse, breaks, contigBorders = the
 *     adjacencies per class; blocks; reverseBlocks = the blocks of direction -1; reverseHits = the hits inside those; largestBlock, in
 *     hits; singletons.  forward + reverse + breaks + contigBorders = count - 1 and blocks = breaks + contigBorders + 1.
 *  6. Block record.  refSeqId (the sketch's own set-global contig id); refStartFirst, refStartLast = p of the block's first and last hit in
 *     bin order; qSeqFirst, qSeqLast = q of the same two hits (qSeqLast > qSeqFirst: forward, <: reverse, equal: singleton); hits; idSum
 *     = the sum of the F[i] of the block.  A pair's blocks come in bin order, `blocks` of them; their hits add up to count and their
 *     idSum to ani_ci_t.sum of the same pair.
 *  7. Order.  The pair records of one call come in the order of that call's rows, restricted to the pairs that pass the gate; the block
 *     records in the same pair order; calls follow each other in call order.
 *  8. Independence.  Rows are untouched.  Nothing depends on schedule, sub-batch size, index chunking, residency or piece sizes.  All
 *     other modes can be on beside it and do not see it; each has its own gate, and the hits' gate and this one may differ in one call.
 * Limits of the statement: query contig borders are not known here (only querySeqId is), so the query's contigs count as one sequence
 * in file order and a draft query shows at most one break per contig border; a circular genome cut at another origin shows one break.
 * begin starts (a second begin drops what is pending and takes the new gate).  take hands over everything appended since begin or the
 * last take and empties both lists: pairs[nPairs] and blocks[nBlocks], each released with ani_free; an empty list comes back NULL with
 * 0.  48 bytes per pair and 32 per block of host memory until taken.  While the mode is on the device holds one more uint32 per cell of
 * a sub-batch's bin table (the hits' owner table, shared with them).  end releases (ani_sketch_destroy does too).  ANI_ERR_ARG: a null
 * sketch (or a null out pointer), a gate outside its ranges (NaN included), take or end without a begin; a refused begin leaves a
 * running mode as it was.  ANI_ERR_NOMEM: the records do not fit the host, or the device cannot hold the table or a piece.
 * ANI_ERR_LIMIT: more than 2^32 - 16 hits, and so blocks, in one (sub-batch, index chunk).  After a call that failed while reducing,
 * the pending lists are unspecified until the next begin. */
typedef struct { int32_t refGenomeId, qryGenomeId; uint32_t count, forward, reverse, breaks, contigBorders, blocks, reverseBlocks,
                 reverseHits, largestBlock, singletons; } ani_synteny_t;   /* 48 bytes */
typedef struct { int32_t refSeqId, refStartFirst, refStartLast, qSeqFirst, qSeqLast; uint32_t hits; uint64_t idSum; } ani_synblock_t;  /* 32 bytes */
int ani_sketch_synteny_begin(ani_sketch *sk, float minIdentity, int32_t minFragments);
int ani_sketch_synteny_take(ani_sketch *sk, ani_synteny_t **pairs, size_t *nPairs, ani_synblock_t **blocks, size_t *nBlocks);
int ani_sketch_synteny_end(ani_sketch *sk);

/* ---- greedy species clustering of the pair graph (no counterpart in the reference, which stops at the rows and the .matrix file;
 * DESIGN.md section 2.11).  Rows' qryGenomeId / refGenomeId are ids in ONE numbering [0, nGenomes) (the command line uses the .matrix
 * numbering); the rows of a pair are folded in the order given (the first sets w, every later one w = (w + identity) / 2 in float),
 * self rows are ignored.  {i, j} is an edge iff w(i, j) >= minIdentity.  Genomes are taken in id order: i is a representative iff no
 * representative j < i has an edge to i; a member goes to the adjacent representative with the largest w, the smallest id on a tie.
 * representative[i] = i for representatives; identityToRep[i] = w(i, representative[i]), 0 for representatives.
 * ANI_ERR_ARG: an id outside [0, nGenomes) or minIdentity outside (0, 100]; ANI_ERR_LIMIT: n > 2^32 - 16 rows, or more than 2^32 - 16
 * edge ends (twice the pairs at or above minIdentity).  n = 0: every genome is its own representative. */
int ani_cluster_greedy(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float minIdentity,
                       int32_t *representative, float *identityToRep);

/* ---- average-linkage (UPGMA) tree of the genomes (no counterpart in the reference).  Rows as for
 * ani_cluster_greedy: ids in ONE numbering [0, nGenomes), the rows of a pair folded in the order given into w(i, j), self rows ignored.
 * Leaf distances: d(i, j) = (float)(1 - (double)w / 100) for a pair with rows, (float)(1 - (double)missingIdentity / 100) without.
 * Clusters live in slots 0..nGenomes-1 (slot i starts as leaf i, size 1).  Merge s = 0..nGenomes-2 takes the active slots a < b with
 * the smallest d(a, b) (ties: the smallest a, then the smallest b), merges b into slot a, retires b, and sets for every other active
 * slot k d(a, k) = (float)((na * (double)d(a, k) + nb * (double)d(b, k)) / (double)(na + nb)), na and nb the cluster sizes.
 * Output in scipy linkage form: merge s creates cluster id nGenomes + s (a leaf's id is its index); children[2s], children[2s + 1]
 * are the ids of the two merged clusters, the smaller first; height[s] is d(a, b) at the merge (non-decreasing in s).
 * children holds 2 (nGenomes - 1) values, height nGenomes - 1.  nGenomes <= 1: ANI_OK, nothing is read or written.
 * ANI_ERR_ARG: a null pointer, nGenomes < 0, an id outside [0, nGenomes), a row identity outside (0, 100] (NaN included), or
 * missingIdentity outside [0, 100]; ANI_ERR_LIMIT: nGenomes > 65536 or n > 2^32 - 16 rows (checked before any allocation);
 * ANI_ERR_NOMEM: the device cannot hold the nGenomes^2 float matrix. */
int ani_tree_average(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                     int32_t *children, float *height);

/* ---- neighbour-joining tree of the genomes (Saitou & Nei, the Q criterion of Studier & Keppler; no counterpart in the reference;
 * DESIGN.md section 2.13).  Defined on fixed-point integers, where the row sums and the criterion are exact, so that the result does
 * not depend on the order of any reduction.
 * 1. Rows and argument checks as for ani_tree_average: ids in ONE numbering [0, nGenomes), the rows of a pair folded in the order given
 *    into w(i, j), self rows ignored.
 * 2. Leaf distance, int32 in units of 2^-24: q(i, j) = (int32) rint((100.0 - (double)w) * 2^24 / 100.0) (round-half-even), with
 *    w = missingIdentity for a pair without rows.
 * 3. Nodes live in slots 0..nGenomes-1 (slot i starts as leaf i); m = active slots; R_i = sum over the active k != i of q(i, k), int64.
 * 4. Join s = 0..nGenomes-3 (m >= 3) takes the active slots a < b with the smallest Q(a, b) = (m - 2) q(a, b) - R_a - R_b (int64);
 *    ties: the smallest a, then the smallest b.
 * 5. Its branch lengths: with t = (double)(R_a - R_b) / (double)(m - 2), len_a = (float)(((double)q(a, b) + t) * 0.5 / 2^24) and
 *    len_b = (float)(((double)q(a, b) - t) * 0.5 / 2^24).  Not clamped: a negative branch (input that is not tree-like) is reported.
 * 6. For every other active slot k, q(a, k) = clamp((q(a, k) + q(b, k) - q(a, b)) >> 1, +-(2^31 - 1)) (the sum in int64, the shift
 *    arithmetic: floor); b is retired; the new node has id nGenomes + s and sits in slot a; R follows.
 * 7. The last record, s = nGenomes - 2 (m = 2), holds the two remaining nodes with len_a = len_b = (float)((double)q(a, b) * 0.5 / 2^24);
 *    for nGenomes >= 3 one of them is the node of join nGenomes - 3.
 * 8. children[2s], children[2s + 1] are the ids of the two nodes of record s, the smaller id first; length[2s], length[2s + 1] the
 *    branch above each, in that order.  children and length hold 2 (nGenomes - 1) values each.  nGenomes <= 1: ANI_OK, nothing is
 *    read or written.
 * Errors and limits as for ani_tree_average; ANI_ERR_NOMEM: the device cannot hold the nGenomes^2 int32 matrix (and the compacted
 * copy, 0.77 of it, that the joins move to). */
int ani_tree_nj(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                int32_t *children, float *length);

/* ---- single-linkage tree of the genomes and the minimum spanning tree of the pair graph (no counterpart in the reference; DESIGN.md
 * section 2.15).  The one linkage that is a function of the pairs with rows alone: device memory is proportional to the rows plus the
 * genomes, never to nGenomes^2, and there is no 65 536 ceiling.  The result depends on no reduction order and no schedule.
 * 1. Rows and argument checks as for ani_tree_average: ids in ONE numbering [0, nGenomes), the rows of a pair folded in the order given
 *    into w(i, j), self rows ignored, the same ANI_ERR_ARG cases.
 * 2. Leaf distance, a float: dm = (float)(1 - (double)missingIdentity / 100); a pair with rows has
 *    d = min((float)(1 - (double)w / 100), dm), a pair without rows d = dm.  The clamp is the one deliberate difference from
 *    ani_tree_average: a pair with a row is never farther than a pair without.  At missingIdentity = 0 (the command line's) it changes
 *    nothing.
 * 3. The merges are Kruskal's over all nGenomes (nGenomes - 1) / 2 pairs in ascending order of (bits(d), lo, hi), lo < hi the leaf ids
 *    (distances are >= 0, so their bit patterns order like their values): a pair whose leaves are already in one cluster is skipped,
 *    every other pair is a merge.
 * 4. Output in scipy linkage form, as for ani_tree_average: merge s = 0..nGenomes-2 creates cluster id nGenomes + s (a leaf's id is its
 *    index); children[2s], children[2s + 1] are the ids of the two merged clusters, the smaller first; height[s] = d of the pair
 *    (non-decreasing in s by construction); edges[2s] = lo and edges[2s + 1] = hi of the pair that caused merge s.  children and edges
 *    hold 2 (nGenomes - 1) values, height nGenomes - 1; edges may be null.
 * 5. A consequence of rule 3, and what lets the implementation stay sparse: at height dm every pair not yet joined is an edge and
 *    (0, k) sorts first, so all merges at height dm are joins to leaf 0: each remaining cluster is joined to the cluster of leaf 0 in
 *    ascending order of its smallest leaf k, with edges = (0, k).  The merges with bits(d) < bits(dm) are exactly the minimum spanning
 *    forest of the pairs with rows under the strict total order (bits(d), lo, hi), so that forest is unique.
 * 6. nGenomes <= 1: ANI_OK, nothing is read or written.  ANI_ERR_LIMIT: n > 2^32 - 16 rows, or nGenomes > 2^30 (cluster ids reach
 *    2 nGenomes - 2 and are int32); ANI_ERR_NOMEM: the device cannot hold the buffers, 56 bytes per row at the peak plus 24 per genome.
 *    All argument and limit checks run before any allocation.
 * ani_tree_single_rounds: the spanning-forest rounds (Boruvka's, at most ceil(log2 nGenomes) + 1) the context's last ani_tree_single
 * call took on the device (or the folds of its last ani_tree_single_sketch call, together); 0 if it needed none or there was no call (tools/tree_probe.py reports it). */
int ani_tree_single(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                    int32_t *children, float *height, int32_t *edges);
int ani_tree_single_rounds(const ani_ctx *ctx);

/* ---- clade support of a tree over replicate trees (no counterpart in the reference).  A pure host function:
 * no context.
 *  1. Inputs.  Every tree is in the record form ani_tree_average, ani_tree_single and ani_tree_nj return: record s names two node ids, a
 *     leaf's id is its index, record s creates node nGenomes + s.  L(leaf) = {leaf}; L(nGenomes + s) is the union of the leaf sets of the
 *     record's two nodes, for every record, NJ's last one included.  children: 2 (nGenomes - 1) ids, the main tree; repChildren:
 *     nReplicates such lists one after the other.
 *  2. Rooted (unrooted = 0; average, single).  support[s] = the number of replicates that have a node u with L(u) = L(nGenomes + s).  The
 *     last record's set is all leaves: its support is nReplicates.
 *  3. Unrooted (unrooted != 0; NJ).  A node stands for the split {L, all \ L}: support[s] = the number of replicates with a node u,
 *     leaves included, where L(u) = L(v) or L(u) = all \ L(v), v = nGenomes + s.  Splits with |L| >= nGenomes - 1 are trivial and get
 *     nReplicates.  The same unrooted tree written with another last join therefore gets full support.
 *  4. Exact: integers, no hashing of leaf sets.  Leaves are numbered in the main tree's traversal order, so a main clade is an interval
 *     of numbers; a replicate node matches iff max - min + 1 = size and that interval is a main clade's (Day 1985), looked up in the sorted
 *     list of the main clades' intervals: O(nGenomes log nGenomes) per replicate, the records walked in their order: no recursion,
 *     whatever the depth.
 *  5. nGenomes <= 1: ANI_OK, nothing is read or written.  nReplicates = 0: every support is 0.  ANI_ERR_ARG: a null pointer, a negative
 *     count, or a record list that is not a tree (an id outside [0, nGenomes + s) in record s, or an id used twice).  ANI_ERR_NOMEM: host. */
int ani_tree_support(const int32_t *children, int32_t nGenomes, const int32_t *repChildren /* [nReplicates][2 (nGenomes - 1)] */,
                     int32_t nReplicates, int32_t unrooted, uint32_t *support /* [nGenomes - 1] */);

/* ---- bootstrap support of an ANI tree: the composition, bit for bit, of nReplicates tree calls and ani_tree_support.  For r in
 * 0 .. nReplicates - 1 the method's entry point (ANI_TREE_AVERAGE: ani_tree_average, ANI_TREE_NJ: ani_tree_nj, ANI_TREE_SINGLE:
 * ani_tree_single) runs on the rows with identity := repIdentity[i * nReplicates + r] for row i; then ani_tree_support runs on `children`
 * — the caller's main tree, normally the same entry point's over the rows as they are — and the nReplicates results, unrooted for NJ.
 * repIdentity comes from ani_sketch_boot_take by the boot records' rule 3, joined to the rows by the caller.  A row that no replicate
 * record covers (a fill row, a row below the boot gate) gets its own identity in every column: it does not vary.  The argument checks
 * and limits are the tree calls' own; a repIdentity outside (0, 100] (NaN included), nReplicates < 0 or an unknown method is ANI_ERR_ARG;
 * all checks run before any tree is made or any device memory taken (the check of `children` takes 2 nGenomes bytes of the host).  nGenomes <= 1: ANI_OK, nothing is read or written.  Host: a copy of the rows and
 * nReplicates record lists. */
#define ANI_TREE_AVERAGE 0
#define ANI_TREE_NJ 1
#define ANI_TREE_SINGLE 2
int ani_tree_support_bootstrap(ani_ctx *ctx, int32_t method, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                               const float *repIdentity /* [n][nReplicates] */, int32_t nReplicates,
                               const int32_t *children, uint32_t *support /* [nGenomes - 1] */);

/* ---- whole-genome sketch ANI: a Mash-style estimate between the reference genomes from the minimizers the sketch already holds (no
 * counterpart in the reference, which emits no row below about 80 % identity).  The smallest k-mer hashes of a
 * genome are almost always window minimizers, so the smallest distinct minimizer hashes of a genome stand in for its bottom-s MinHash
 * sketch.  Integers only: the result depends on no reduction order and no scheduling.
 * 1. The signature of genome g at `size` (1 <= size <= 4096) is the ascending list of the `size` smallest distinct `hash` values among
 *    the sketch's minimizer records whose seqId belongs to g; all of them if there are fewer.  len(g) = min(size, distinct hashes of g),
 *    which can be 0.
 * 2. A pair (a, b), a < b: U = the ascending distinct union of the two signatures; size(a, b) = min(size, |U|); shared(a, b) = the
 *    number of values among the first size(a, b) of U that occur in both signatures.
 * 3. identity(a, b), by the library on the host: 0 if shared = 0, else
 *    100.0 * (1.0 + log(2.0 * shared / (double)(size(a, b) + shared)) / kmerSize) in double, clamped to [0, 100], rounded once to float
 *    (the Mash distance -ln(2 j / (1 + j)) / k at j = shared / size).
 * ani_sketch_signatures: every sketch the library can hold (built, loaded, from record parts; one or several index chunks; resident or
 * streamed) — it reads the index arrays or the kept records, whichever are at hand, and rebuilds nothing.  sig[g * size ..] is row g,
 * ascending, the unused tail 0; ids are the sketch's own (0 .. nGenomes - 1).  ANI_ERR_ARG: a null pointer, size outside [1, 4096].
 * ani_signature_pairs: rows as ani_sketch_signatures lays them out (from one sketch or collected from several), genome ids = row
 * numbers.  Returns the pairs with shared >= minShared (0: every pair), ordered by (a, b); ani_free releases *rows.  nGenomes of 0 or 1:
 * no rows.  ANI_ERR_ARG: a null pointer, nGenomes < 0, size outside [1, 4096], kmerSize outside [1, 16], minShared < 0, a len outside
 * [0, size], a row that does not ascend strictly inside its len; ANI_ERR_LIMIT: nGenomes > 65536 (arguments and limits are checked
 * before anything is allocated); ANI_ERR_NOMEM: the device cannot hold the nGenomes^2 uint32 result matrix (or the host the rows). */
typedef struct { int32_t a, b, shared, size; float identity; } ani_sigpair_t;
int ani_sketch_signatures(const ani_sketch *sk, int32_t size, uint32_t *sig /* [nGenomes * size] */, int32_t *len /* [nGenomes] */);
int ani_signature_pairs(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize,
                        int32_t minShared, ani_sigpair_t **rows, size_t *n);

/* ---- single-linkage tree of the rows with the whole-genome sketch estimate for every pair without rows, streamed (no counterpart in the
 * reference).  ani_tree_single over the rows and the fill of ani_signature_pairs in one call that never holds
 * anything of size nGenomes^2, on the device or on the host: there is no 65 536 ceiling.
 * 1. Defined by composition.  P = the pairs ani_signature_pairs(sig, len, nGenomes, size, kmerSize, minShared) returns.  F = the pairs
 *    of P with identity > 0 that have no row in `rows` other than self rows (rows of either direction count, whatever their identity).
 *    children, height and edges are those of ani_tree_single over `rows` followed by one row (a, b, identity) per pair of F, at the same
 *    missingIdentity.  The order of F does not matter: a pair of F has one row.
 * 2. source[s], one byte per merge: 0 if the pair that caused merge s has rows, 1 if it is a pair of F, 2 for a join to leaf 0 at the
 *    missing distance (ani_tree_single's rule 5).  source may be null, and so may edges.
 * 3. rows, nGenomes, missingIdentity, children, height, edges: as for ani_tree_single.  sig, len, size, kmerSize: as for
 *    ani_signature_pairs, genome ids = row numbers = the ids of `rows`.  minShared >= 1.
 * 4. ANI_ERR_ARG: every case of ani_tree_single (a null pointer, nGenomes < 0, an id outside [0, nGenomes), a row identity outside
 *    (0, 100], missingIdentity outside [0, 100]) and of ani_signature_pairs (size outside [1, 4096], kmerSize outside [1, 16], a len
 *    outside [0, size], a signature that does not ascend strictly inside its len), and minShared < 1.  ANI_ERR_LIMIT: ani_tree_single's
 *    own, n > 2^32 - 16 rows or nGenomes > 2^30.  The checks of the scalar arguments and of len run before any allocation.
 * 5. nGenomes <= 1: ANI_OK, nothing is read or written.
 * 6. Memory.  The sketch pairs are made a strip of rows of the pair matrix at a time and folded into a forest of at most nGenomes - 1
 *    edges.  Device: ani_tree_single's for the rows, 8 size nGenomes bytes while the signatures are staged (half of it after), 2 size^2
 *    bytes of distances, 8 bytes per pair with rows, and one strip, whose height follows the free device memory.  Host: 13 bytes per
 *    forest edge.  ANI_TEST_SIG_STRIP_ROWS (tests) forces a strip height; the result does not depend on it.
 * ani_tree_single_rounds counts the spanning-forest rounds of all folds of the call.  ani_tree_single_sketch_strips: the strips of the
 * context's last call (its return value) and, for the first `cap` of them, the edges each strip added to its fold (may be null). */
int ani_tree_single_sketch(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                           const uint32_t *sig, const int32_t *len, int32_t size, int32_t kmerSize, int32_t minShared,
                           int32_t *children, float *height, int32_t *edges /* may be null */, uint8_t *source /* may be null */);
int ani_tree_single_sketch_strips(const ani_ctx *ctx, uint64_t *edgesPerStrip, size_t cap);

/* ---- nearest neighbours of every genome under the whole-genome sketch estimate, streamed (no counterpart in the reference; DESIGN.md
 * section 2.17).  For each genome of a range of rows, its k closest relatives among all genomes and how close they are: O(n k) of output
 * from the O(n^2) comparisons, which never leave the device.  There is no 65 536 ceiling.
 * 1. Defined by composition.  P = the pairs ani_signature_pairs(sig, len, nGenomes, size, kmerSize, minShared) would return, were it free
 *    of its ceiling; shared, size and identity of a pair are exactly its rules 2 and 3.
 * 2. The candidates of genome g are the pairs of P that contain g and have identity >= minIdentity; the other genome of the pair is the
 *    neighbour.
 * 3. Candidates are ordered by identity descending, then neighbour id ascending.  Identities are non-negative floats, so the order of
 *    their values is the order of their bit patterns; a minIdentity of -0.0 is 0.
 * 4. count[g - rowBegin] = min(k, candidates of g).
 * 5. out[(g - rowBegin) * k + i] is the i-th candidate of g, for i < count[g - rowBegin].
 * 6. The unused slots of a list are {-1, 0, 0, 0.0f}.
 * 7. Only the genomes of [rowBegin, rowEnd) get lists; their neighbours come from all of [0, nGenomes).  Rows are independent: a caller
 *    may split the range, or ask for new genomes only.
 * 8. ANI_ERR_ARG: a null pointer, nGenomes < 0, size outside [1, 4096], kmerSize outside [1, 16], minShared < 1, minIdentity outside
 *    [0, 100] (NaN included), k outside [1, 1024], not 0 <= rowBegin <= rowEnd <= nGenomes, a len outside [0, size], a signature that
 *    does not ascend strictly inside its len.
 * 9. ANI_ERR_LIMIT: nGenomes > 2^30.
 * 10. The checks of the scalar arguments run before any allocation.
 * 11. nGenomes == 0 or rowBegin == rowEnd: ANI_OK after the scalar checks, nothing is read or written; sig, len, out and count may
 *    then be null.
 * 12. The result depends on no schedule, no reduction order and no strip height.
 * 13. Memory.  The rows of the range go through the device a strip at a time.  Device: 8 size nGenomes bytes while the signatures are
 *    staged (half of it after), 2 size^2 bytes of identities, one strip of rows x nGenomes 4-byte cells, whose height follows the free
 *    device memory, and 16 k + 4 bytes per row of the range.  Nothing follows nGenomes^2.  ANI_TEST_SIG_STRIP_ROWS (tests) forces a
 *    strip height.
 * ani_signature_neighbors_strips: the strips the context's last ani_signature_neighbors call took; 0 if it needed none or there was no
 * call (tools/sketch_probe.py reports it). */
typedef struct { int32_t neighbor, shared, size; float identity; } ani_signeighbor_t;   /* 16 bytes */
int ani_signature_neighbors(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize,
                            int32_t minShared, float minIdentity, int32_t k, int32_t rowBegin, int32_t rowEnd,
                            ani_signeighbor_t *out /* [(rowEnd - rowBegin) * k] */, int32_t *count /* [rowEnd - rowBegin] */);
int ani_signature_neighbors_strips(const ani_ctx *ctx);

/* ---- screening of query genomes against reference genomes under the whole-genome sketch estimate, streamed (no counterpart in the
 * reference).  For each query its k closest references and how close they are: a few new genomes against a
 * large fixed set.  The two sets are separate arrays, and only pairs of a query and a reference are compared.
 * 1. Defined by composition.  C = the signatures of the nRef references followed by the nQry queries, laid out as ani_sketch_signatures
 *    lays out rows.  P = the pairs ani_signature_pairs(C, nRef + nQry, size, kmerSize, minShared) would return, were it free of its
 *    ceiling; shared, size and identity of a pair are exactly its rules 2 and 3.
 * 2. The candidates of query q are the pairs (r, nRef + q) of P with r < nRef and identity >= minIdentity; the neighbour is r, a
 *    reference id.  Pairs between two queries or between two references play no part.  A query whose signature equals a reference's is
 *    a candidate of that reference at identity 100.
 * 3. Order, cut, records and unused slots are rules 3 - 6 of ani_signature_neighbors: identity descending, by bit pattern, then
 *    reference id ascending; count[q] = min(k, candidates of q); out[q * k + i] is the i-th candidate of q for i < count[q]; the unused
 *    slots are {-1, 0, 0, 0.0f}; a minIdentity of -0.0 is 0.
 * 4. ANI_ERR_ARG: a null pointer, nRef < 0 or nQry < 0, size outside [1, 4096], kmerSize outside [1, 16], minShared < 1, minIdentity
 *    outside [0, 100] (NaN included), k outside [1, 1024], a len outside [0, size], a signature in either set that does not ascend
 *    strictly inside its len.
 * 5. ANI_ERR_LIMIT: nRef > 2^30 or nQry > 2^30.  The checks of the scalar arguments run before any allocation.
 * 6. nQry == 0: ANI_OK after the scalar checks, nothing is read or written; the array pointers may then be null.  nRef == 0 with
 *    nQry > 0: every count is 0 and every slot is unused; refSig and refLen may be null.
 * 7. The result depends on no schedule, no reduction order, no strip height and no tile shape.
 * 8. Memory.  The reference signatures are staged once; the queries go through the device a strip at a time.  Device: 8 size bytes per
 *    genome of either set while it is staged (half of it after), 2 size^2 bytes of identities, one strip of rows x nRef 4-byte cells,
 *    whose height follows the free device memory, and 16 k + 4 bytes per query.  Nothing follows nRef * nQry, and there is no 65 536
 *    ceiling on either side.  ANI_TEST_SIG_STRIP_ROWS (tests) forces a strip height, ANI_TEST_SIG_SCREEN_SHAPE = square | thin the
 *    shape of the merge tile, which otherwise follows the strip height.
 * 9. ani_signature_screen_strips: the strips the context's last screen call of either kind (ani_signature_screen,
 *    ani_signature_screen_contain) took; 0 if it needed none or there was no call.  ani_signature_screen_tile: the queries x references
 *    of the merge tile of that call's last strip, 0 x 0 likewise (tools/sketch_probe.py reports both). */
int ani_signature_screen(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef,
                         const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                         int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k,
                         ani_signeighbor_t *out /* [nQry * k] */, int32_t *count /* [nQry] */);
int ani_signature_screen_strips(const ani_ctx *ctx);
void ani_signature_screen_tile(const ani_ctx *ctx, int32_t *tileQueries, int32_t *tileRefs);

/* ---- screening under the containment estimate (no counterpart in the reference).  ani_signature_screen's
 * estimate is a Jaccard index over the first `size` values of the union of two signatures: right when query and reference are about
 * the same size and both complete, low for a partial genome, a plasmid or a contig against a whole one, and for a reference inside a
 * much larger assembly.  This call divides the shared values by the part of one signature that lies where the other is complete.
 * Everything is integer except the last step.  Q is a query signature and R a reference signature, ascending distinct lists of lengths
 * lq and lr, as ani_sketch_signatures lays them out at `size`.
 * 1. A signature is truncated iff its length equals `size`: the genome may have more values than the sketch holds.  A shorter
 *    signature is the genome's whole set.
 * 2. shared = the number of values that occur in both lists, over the whole of both: not cut at `size` union elements, unlike rule 2 of
 *    ani_signature_pairs.
 * 3. inQ = the number of values of Q that are <= the last value of R, if R is truncated; otherwise inQ = lq.  inR likewise with the
 *    roles swapped.  These are the parts of each list in the hash range where the other sketch is complete.  Every shared value counts
 *    in both: shared <= inQ <= size, shared <= inR <= size, and shared >= 1 implies both >= 1.
 * 4. mode selects the denominator d.  ANI_CONTAIN_QUERY: d = inQ, how much of the query is in the reference (partial genomes, plasmids,
 *    contigs).  ANI_CONTAIN_REF: d = inR, how much of the reference is in the query (references inside a large assembly).
 *    ANI_CONTAIN_MAX: d = min(inQ, inR), symmetric in the two sets.
 * 5. identity = 0 if shared = 0; otherwise 100.0 * pow((double) shared / (double) d, 1.0 / (double) kmerSize) in double, clamped to
 *    [0, 100] and rounded once to float, by the library on the host.  shared = d gives exactly 100.
 * 6. The candidates of query q are the references r with shared >= minShared and identity >= minIdentity.  Order, cut, count and unused
 *    slots are rules 3 - 6 of ani_signature_neighbors: identity descending by bit pattern, then reference id ascending;
 *    count[q] = min(k, candidates of q); the unused slots are {-1, 0, 0, 0.0f}; a minIdentity of -0.0 is 0.  The record is
 *    ani_signeighbor_t{neighbor = r, shared, size = d, identity}.
 * 7. Errors and limits are rules 4 - 6 of ani_signature_screen, and ANI_ERR_ARG for a mode outside 0 .. 2.  The checks of the scalar
 *    arguments run before any allocation.  nQry == 0: nothing is read or written.  nRef == 0: every list is empty.
 * 8. Memory is rule 8 of ani_signature_screen; ANI_TEST_SIG_STRIP_ROWS and ANI_TEST_SIG_SCREEN_SHAPE act on this call too.  The result
 *    depends on no schedule, no strip height and no tile shape.
 * ani_signature_screen_strips and ani_signature_screen_tile report this call as they report ani_signature_screen. */
typedef enum { ANI_CONTAIN_QUERY = 0, ANI_CONTAIN_REF = 1, ANI_CONTAIN_MAX = 2 } ani_contain_mode;
int ani_signature_screen_contain(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef,
                                 const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                                 int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, int32_t mode,
                                 ani_signeighbor_t *out /* [nQry * k] */, int32_t *count /* [nQry] */);

/* ---- greedy representative clustering of the genomes under the whole-genome sketch estimate, streamed (no counterpart in the
 * reference).  Dereplication: one representative per group of near-identical genomes of a large collection.
 * ani_cluster_greedy over the pairs of ani_signature_pairs in one call that compares a genome with the representatives only, about
 * nGenomes x representatives pairs instead of nGenomes^2 / 2, keeps every pair on the device and returns two records per genome.
 * There is no 65 536 ceiling.
 * 1. Defined by composition.  P = the pairs ani_signature_pairs(sig, len, nGenomes, size, kmerSize, minShared) would return, were it free
 *    of its ceiling; shared, size and identity of a pair are exactly its rules 2 and 3.
 * 2. Edges.  {a, b} is an edge iff the pair is in P and bits(identity) >= bits(minIdentity).  Identities are non-negative floats, so the
 *    order of their values is the order of their bit patterns.  An identity the clamp leaves at 0 is never an edge: minIdentity > 0.
 * 3. Greedy rule.  Genomes are taken in id order, as in ani_cluster_greedy: genome i is a representative iff no representative j < i has
 *    an edge to i; every other genome is a member.  A member goes to the adjacent representative with the largest identity, whatever
 *    its id (a representative with a larger id than the member counts), the smallest id on a tie.
 * 4. Outputs.  representative[i] = i for a representative, otherwise the id rule 3 chose.  link[i] = {representative[i], shared, size,
 *    identity} of that pair for a member, the unused record {-1, 0, 0, 0.0f} for a representative.
 * 5. Equivalence.  representative equals what ani_cluster_greedy returns over one row {refGenomeId = a, qryGenomeId = b, identity} per
 *    pair of P at the same minIdentity, and link[i].identity equals its identityToRep[i] bit for bit for members.
 * 6. ANI_ERR_ARG: a null pointer, nGenomes < 0, size outside [1, 4096], kmerSize outside [1, 16], minShared < 1, minIdentity outside
 *    (0, 100] (NaN included), a len outside [0, size], a signature that does not ascend strictly inside its len.
 * 7. ANI_ERR_LIMIT: nGenomes > 2^30.  The checks of the scalar arguments run before any allocation.
 * 8. nGenomes == 0: ANI_OK after the scalar checks, nothing is read or written; sig, len, representative and link may then be null.
 * 9. The result depends on no schedule, no reduction order, no strip height and no tile shape.
 * 10. Memory.  The genomes go through the device a strip of rows at a time, twice: once in id order to find the representatives, once
 *    for the members against the representatives found after their strip.  Device: 8 size nGenomes bytes while the signatures are
 *    staged (half of it after), the signature rows of the representatives (at most one more copy), 2 size^2 bytes of identities, one
 *    strip of rows x max(representatives, rows) 4-byte cells, whose height follows the free device memory and is capped by the genome
 *    count, and 28 bytes per genome.  Nothing follows nGenomes^2.  ANI_TEST_SIG_STRIP_ROWS (tests) forces a strip height (4096 rows at
 *    the most), ANI_TEST_SIG_SCREEN_SHAPE = square | thin the shape of the merge tile, which otherwise follows the strip height.
 * ani_signature_cluster_stats: of the context's last ani_signature_cluster call, out[0] = its strips, out[1] = its representatives,
 * out[2] = the cells its merge launches covered (rows x references of every launch: strip x earlier representatives, strip x strip,
 * strip x later representatives), out[3] = its resolve steps (sweeps of 256 cells of a representative's row of a strip's own block by
 * the one workgroup that resolves the strip: the sequential part); all 0 if there was no call or it had no genomes
 * (tools/sketch_probe.py reports them).  ANI_ERR_ARG: out is null. */
int ani_signature_cluster(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize,
                          int32_t minShared, float minIdentity,
                          int32_t *representative /* [nGenomes] */, ani_signeighbor_t *link /* [nGenomes] */);
int ani_signature_cluster_stats(const ani_ctx *ctx, uint64_t out[4]);   /* strips, representatives, cells walked, resolve steps of the last call */

/* ---- greedy representative clustering under the containment estimate, streamed (no counterpart in the reference; DESIGN.md section
 * 2.22).  ani_signature_cluster's estimate is a Jaccard index, which reads low for a genome that is partly there: a bin that holds half
 * of a genome shares half of the genome's sketch, shared / size = 1 / 2, which reads 97.5 % at kmerSize 16 (96.5 % for a bin that holds
 * 40 %), and becomes a representative of its own at a threshold of 99.  This call clusters by the share of the smaller genome
 * instead, so that metagenome-assembled genomes of unequal completeness join the genome they are parts of.  The rules are
 * ani_signature_cluster's with another pair.
 * 1. The pair.  For a < b, Q is the signature of a and R the signature of b; shared, inQ, inR, d and identity are exactly rules 1 - 5 of
 *    ani_signature_screen_contain, and so rule 2 of ani_signature_graph: shared over the whole of both lists, d = min(inQ, inR).
 * 2. mode must be ANI_CONTAIN_MAX.  The greedy rule asks whether {a, b} is an edge, not whether a is in b, so it needs an estimate that
 *    is symmetric in the two genomes; ANI_CONTAIN_QUERY and ANI_CONTAIN_REF are ANI_ERR_ARG with a message that says so, and so is
 *    every value outside 0 .. 2.  The argument exists so that the signature stays if a directed rule is defined later.
 * 3. Edges.  {a, b} is an edge iff shared >= minShared and bits(identity) >= bits(minIdentity).
 * 4. The greedy rule, the outputs, the errors, the limits, the nGenomes == 0 case and the independence of schedule, reduction order,
 *    strip height and tile shape are rules 3, 4 and 6 - 9 of ani_signature_cluster; minIdentity lies in (0, 100].  link[i] of a member
 *    is {representative[i], shared, d, identity} of that pair.
 * 5. Equivalence.  representative equals what ani_cluster_greedy returns over one row {refGenomeId = a, qryGenomeId = b, identity} per
 *    record with shared >= minShared of ani_signature_graph(sig, len, nGenomes, size, kmerSize, minShared, 0, ANI_GRAPH_CONTAIN_MAX, 0,
 *    nGenomes), at the same minIdentity, and link[i].identity equals its identityToRep[i] bit for bit for members.
 * 6. Memory is rule 10 of ani_signature_cluster; ANI_TEST_SIG_STRIP_ROWS acts on this call too, and ANI_TEST_SIG_SCREEN_SHAPE on its
 *    rectangular launches.  In mode MAX cell (a, b) equals cell (b, a), so a strip's own rows x rows block is made from its upper
 *    triangle, one walk per pair.  ANI_TEST_SIG_CLUSTER_TRI = 0 (tests, tools/sketch_probe.py) walks the full block instead; the result
 *    does not depend on it.
 * ani_signature_cluster_stats reports the context's last call of either kind.  out[2] counts the cells a launch walked: rows x
 * references of a rectangular launch, and rows (rows - 1) / 2, not rows^2, of a triangular launch over the rows of a strip. */
int ani_signature_cluster_contain(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize,
                                  int32_t minShared, float minIdentity, int32_t mode,
                                  int32_t *representative /* [nGenomes] */, ani_signeighbor_t *link /* [nGenomes] */);

/* ---- the pair graph of the genomes under either whole-genome sketch estimate, streamed (no counterpart in the reference; DESIGN.md
 * section 2.21).  The pair list of ani_signature_pairs, filtered on the device by an identity threshold and made a strip of rows at a
 * time: what clustering and graph tools take as their input.  There is no 65 536 ceiling, and containment is available for all pairs.
 * 1. ANI_GRAPH_MASH: shared, size and identity of a pair (a, b), a < b, are exactly rules 2 and 3 of ani_signature_pairs, were it free
 *    of its ceiling.
 * 2. ANI_GRAPH_CONTAIN_MAX: Q is the signature of a and R the signature of b; shared, inQ, inR, d = min(inQ, inR) and identity are
 *    exactly rules 1 - 5 of ani_signature_screen_contain in mode ANI_CONTAIN_MAX.  This is symmetric, so which genome is Q does not
 *    matter.  The record's `size` field holds d.
 * 3. A pair is kept iff shared >= minShared and bits(identity) >= bits(minIdentity).  Identities are non-negative floats, so the order
 *    of their values is the order of their bit patterns; a minIdentity of -0.0 is 0.  At minIdentity = 0 a pair that the clamp leaves at
 *    identity 0 is kept: at ANI_GRAPH_MASH, minIdentity 0 and the full range the call returns exactly the records of ani_signature_pairs.
 * 4. *rows holds the kept pairs with rowBegin <= a < rowEnd and b > a, b over all of (a, nGenomes), ordered by (a, b).  The identity is
 *    the float the host arithmetic of the defining call yields, bit for bit.  ani_free releases *rows.  Row ranges are independent, and
 *    the concatenation of the results of a split range is the result of the whole range.
 * 5. ANI_ERR_ARG: a null pointer, nGenomes < 0, size outside [1, 4096], kmerSize outside [1, 16], minShared < 1, minIdentity outside
 *    [0, 100] (NaN included), estimate outside 0 .. 1, not 0 <= rowBegin <= rowEnd <= nGenomes, a len outside [0, size], a signature
 *    that does not ascend strictly inside its len.
 * 6. ANI_ERR_LIMIT: nGenomes > 2^30, or more than 2^32 - 16 kept pairs in the range: the caller splits the range.  The checks of the
 *    scalar arguments run before any allocation.
 * 7. nGenomes <= 1 or rowBegin == rowEnd: ANI_OK after the scalar checks, *rows = NULL and *n = 0; nothing else is read, and sig and len
 *    may then be null.  A range without a kept pair also yields *rows = NULL and *n = 0.
 * 8. The result depends on no schedule, no reduction order and no strip height.
 * 9. Memory.  The rows of the range go through the device a strip at a time.  Device: 8 size nGenomes bytes while the signatures are
 *    staged (half of it after), as ani_signature_neighbors stages them, 2 size^2 bytes of identity bits, one strip of rows x nGenomes
 *    4-byte cells, whose height follows the free device memory, 4 bytes per row of a strip for each of its counts and offsets, and 20
 *    bytes per kept pair of a strip.  Host: 20 bytes per kept pair of the range.  Nothing follows nGenomes^2.  ANI_TEST_SIG_STRIP_ROWS
 *    (tests) forces a strip height.
 * ani_signature_graph_strips: the strips the context's last ani_signature_graph call took; 0 if it needed none or there was no call
 * (tools/sketch_probe.py reports it). */
typedef enum { ANI_GRAPH_MASH = 0, ANI_GRAPH_CONTAIN_MAX = 1 } ani_graph_estimate;
int ani_signature_graph(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize,
                        int32_t minShared, float minIdentity, int32_t estimate, int32_t rowBegin, int32_t rowEnd,
                        ani_sigpair_t **rows, size_t *n);
int ani_signature_graph_strips(const ani_ctx *ctx);

/* ---- synthetic genomes (benchmark input generator; DESIGN.md §Synthetic data) ----
 * Writes nGenomes genomes of genomeLen bases, 2-bit packed, genome i at word offset i*ceil(genomeLen/16) of devOut
 * (device memory, caller-allocated).  `variant` re-draws the substitutions with the cluster ancestors kept (0 = base set). */
int ani_synth_packed(ani_ctx *ctx, uint64_t seed, uint64_t variant, int32_t firstGenomeId, int32_t nGenomes, int32_t genomeLen, void *devOut);
/* the same population with clusters of `clusterSize` related genomes instead of 20 (a species-dense database: hundreds of strains of
 * one species; members beyond the 20th cycle through the non-zero divergence rates) */
int ani_synth_packed_clusters(ani_ctx *ctx, uint64_t seed, uint64_t variant, int32_t firstGenomeId, int32_t nGenomes, int32_t genomeLen,
                              int32_t clusterSize, void *devOut);

#ifdef __cplusplus
}
#endif
#endif
