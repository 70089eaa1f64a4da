// engine_sig.hip — the whole-genome sketch estimate that fills the pairs the mapping leaves without a row: signatures of the reference
// genomes and their all-pairs comparison (ani_sketch_signatures, ani_signature_pairs, kernels/sigdist.hpp), and its streamed consumers: the
// single-linkage tree with sketch fill (ani_tree_single_sketch, kernels/sigstrip.hpp, over the pieces of engine_graph.hip), neighbours
// (kernels/signeigh.hpp), screens (kernels/sigscreen.hpp, kernels/sigcontain.hpp), the greedy clustering of ani_signature_cluster and
// ani_signature_cluster_contain (kernels/sigcluster.hpp) and the pair graph of ani_signature_graph (kernels/siggraph.hpp).
#include "host/engine.hpp"
#include "kernels/sigdist.hpp"
#include "kernels/sigstrip.hpp"
#include "kernels/signeigh.hpp"
#include "kernels/sigscreen.hpp"
#include "kernels/sigcontain.hpp"
#include "kernels/sigcluster.hpp"
#include "kernels/siggraph.hpp"

namespace anih {
using namespace ani;

// ---- whole-genome sketch ANI (ani_sketch_signatures, ani_signature_pairs) ----
// Per index chunk, from whichever form of its records is at hand (the index arrays of a resident chunk, else the 12-byte records a
// streamed set keeps: nothing is rebuilt).  Round 1 keeps the records at or below a per-genome hash threshold that lets about
// 2 size + 64 k-mers of the genome through (a k-mer that small is a window minimizer almost surely), sorts those few keys and numbers
// the distinct ones; a genome that yields fewer than `size` that way (repeats, a short genome) goes through round 2 with every record.
// Device memory: 8 bytes per genome, 4 + 4 per block of 2048 records, 2 x 8 bytes per kept record plus the sort's workspace,
// 4 (size + 1) per genome for the result.
int sketch_signatures(const ani_sketch *sk, int32_t size, uint32_t *sig, int32_t *len)
{
  enum { THR, CNT, OFF, KEYS_A, KEYS_B, SORT, SIG, LEN, NBUF };
  DevBufs B(NBUF);
  ani_ctx *ctx = sk->ctx;
  hipStream_t st = ctx->stream;
  const int64_t kAll = 0xffffffffll;
  for (const IndexChunk *ch : sk->chunks) {
    const int32_t nG = ch->nGenomes;
    if (nG <= 0) continue;
    std::vector<SigSource> src;
    if (ch->n) {
      if (ch->resident) src.push_back(SigSource{ch->mHash, ch->mSeq, 1u, 0, (uint64_t)ch->n});
      else for (const RecordPiece &pc : ch->pieces) if (pc.n) src.push_back(SigSource{pc.rec, (const int32_t *)pc.rec + 1, 3u, ch->c0, (uint64_t)pc.n});
      if (src.empty()) return fail(ANI_ERR_INTERNAL, "index chunk of genomes [%d, %d) holds neither index arrays nor records", ch->g0, ch->g0 + nG);
    }
    uint64_t nBlocks = 0;
    for (const SigSource &s : src) nBlocks += (s.n + kSigBlock - 1) / kSigBlock;
    std::vector<int64_t> thr((size_t)nG);
    const uint64_t want = 2 * (uint64_t)size + 64;
    for (int32_t g = 0; g < nG; g++) {
      uint64_t bases = 0;
      for (int32_t c = sk->genomeContigStart[(size_t)(ch->g0 + g)]; c < sk->genomeContigStart[(size_t)(ch->g0 + g) + 1]; c++) bases += (uint64_t)sk->contigLen[(size_t)c];
      const uint64_t recs = sk->genomeRecStart[(size_t)(ch->g0 + g) + 1] - sk->genomeRecStart[(size_t)(ch->g0 + g)];
      thr[(size_t)g] = (bases <= want || recs <= want) ? kAll : (int64_t)std::min<uint64_t>((uint64_t)kAll, (want << 32) / bases);
    }
    int64_t *dThr; int32_t *dCnt, *dLen; uint32_t *dOff, *dSig;
    TRY(B.get(THR, (size_t)nG * 8, (void **)&dThr)); TRY(B.get(CNT, nBlocks * 4, (void **)&dCnt)); TRY(B.get(OFF, nBlocks * 4, (void **)&dOff));
    TRY(B.get(SIG, (size_t)nG * (size_t)size * 4, (void **)&dSig)); TRY(B.get(LEN, (size_t)nG * 4, (void **)&dLen));
    std::vector<int32_t> hostLen((size_t)nG);
    const int bits = id_bits(nG);
    for (int round = 0; round < 2; round++) {
      HIP_TRY(hipMemcpyAsync(dThr, thr.data(), (size_t)nG * 8, hipMemcpyHostToDevice, st));
      uint64_t total = 0, at = 0;
      for (const SigSource &s : src) {
        const uint64_t nb = (s.n + kSigBlock - 1) / kSigBlock;
        hipLaunchKernelGGL(k_sig_count, dim3((unsigned)nb), dim3(kTPB), 0, st, s, (const int32_t *)ch->contigGenome, (const int64_t *)dThr, dCnt + at);
        at += nb;
      }
      HIP_TRY(hipGetLastError());
      if (nBlocks) TRY(device_scan(ctx, dCnt, dOff, (uint32_t)nBlocks, &total));
      uint64_t *keysA, *keysB;
      TRY(B.get(KEYS_A, (size_t)total * 8, (void **)&keysA)); TRY(B.get(KEYS_B, (size_t)total * 8, (void **)&keysB));
      if (total) {
        at = 0;
        for (const SigSource &s : src) {
          const uint64_t nb = (s.n + kSigBlock - 1) / kSigBlock;
          hipLaunchKernelGGL(k_sig_keys, dim3((unsigned)nb), dim3(kTPB), 0, st, s, (const int32_t *)ch->contigGenome, (const int64_t *)dThr,
                             (const uint32_t *)dOff + at, keysA);
          at += nb;
        }
        HIP_TRY(hipGetLastError());
        size_t tb = 0;
        int rc = ani_sort_keys_u64_bits(keysA, keysB, (size_t)total, 32 + bits, nullptr, &tb, st);
        void *sortTmp = nullptr;
        if (rc == 0) { TRY(B.get(SORT, tb + 256, &sortTmp)); rc = ani_sort_keys_u64_bits(keysA, keysB, (size_t)total, 32 + bits, sortTmp, &tb, st); }
        if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the signature keys failed (%d)", rc);
      }
      hipLaunchKernelGGL(k_sig_emit, dim3((unsigned)nG), dim3(kTPB), 0, st, (const uint64_t *)keysB, (uint32_t)total, (const int64_t *)dThr, size, dSig, dLen);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hostLen.data(), dLen, (size_t)nG * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      bool again = false;
      for (int32_t g = 0; g < nG && round == 0; g++) {
        const bool more = hostLen[(size_t)g] < size && thr[(size_t)g] >= 0 && thr[(size_t)g] != kAll;
        thr[(size_t)g] = more ? kAll : -1;
        again = again || more;
      }
      if (!again) break;
    }
    HIP_TRY(hipMemcpyAsync(sig + (size_t)ch->g0 * (size_t)size, dSig, (size_t)nG * (size_t)size * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(len + ch->g0, hostLen.data(), (size_t)nG * 4);
  }
  return ANI_OK;
}

// identity of a pair from its exact integers (ani_abi.h): one double expression, rounded once
static inline float sig_identity(int32_t shared, int32_t size, int32_t kmerSize)
{
  if (shared == 0) return 0.0f;
  double id = 100.0 * (1.0 + log(2.0 * (double)shared / (double)(size + shared)) / (double)kmerSize);
  if (id < 0.0) id = 0.0;
  if (id > 100.0) id = 100.0;
  return (float)id;
}

// identity of a pair under the containment estimate from its exact integers (ani_signature_screen_contain, rule 5): one double
// expression, rounded once
static inline float sig_contain_identity(int32_t shared, int32_t d, int32_t kmerSize)
{
  if (shared == 0) return 0.0f;
  double id = 100.0 * pow((double)shared / (double)d, 1.0 / (double)kmerSize);
  if (id < 0.0) id = 0.0;
  if (id > 100.0) id = 100.0;
  return (float)id;
}

// ---- the steps the streamed calls share ----
namespace {
// a strip takes this share of the device memory that is free when its height is chosen
constexpr double kSigStripShare = 0.5;
constexpr uint64_t kNoStripCap = ~0ull;                               // sig_strip_rows: no cap before the forced height

// One set of signatures to the device: as given, then at a pitch of whole quads by k_sigpair_stage, which sets bit 0 of dFlags[0] (zeroed
// by the caller, who may stage several sets against it) for a row that does not ascend.  The raw copy is released before the return.
int sig_stage(ani_ctx *ctx, DevBuf &raw, DevBuf &staged, DevBuf &lens, const uint32_t *sig, const int32_t *len, size_t n, int32_t size, int32_t pitch,
              uint32_t *dFlags)
{
  hipStream_t st = ctx->stream;
  TRY(raw.ensure(n * (size_t)size * 4)); TRY(staged.ensure(n * (size_t)pitch * 4)); TRY(lens.ensure(n * 4));
  HIP_TRY(hipMemcpyAsync(raw.p, sig, n * (size_t)size * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(lens.p, len, n * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sigpair_stage, dim3((unsigned)n), dim3(kTPB), 0, st, (const uint32_t *)raw.p, (const int32_t *)lens.p, size, pitch, staged.as<uint32_t>(), dFlags);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));                                   // (sig and len are the caller's pageable memory)
  raw.release();
  return ANI_OK;
}

// what the sets staged against dFlags left there, read through the pinned slot
int sig_stage_check(ani_ctx *ctx, const uint32_t *dFlags)
{
  uint32_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));
  HIP_TRY(hipMemcpyAsync(host, dFlags, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (host[0] & 1u) return fail(ANI_ERR_ARG, "a signature does not ascend strictly");
  return ANI_OK;
}

// bits(identity) of every (shared, size') with 1 <= shared <= size' <= size: rule 3 in double on the host; `contain`: of every (shared, d)
// under the containment estimate instead, in the same triangular layout
std::vector<uint32_t> sig_identity_table(int32_t size, int32_t kmerSize, bool contain)
{
  const size_t S = (size_t)size;
  std::vector<uint32_t> table(S * (S + 1) / 2);
  parallel_for(S, (uint64_t)table.size() * 64, [&](size_t i) {
    const int32_t sz = (int32_t)i + 1;
    for (int32_t sh = 1; sh <= sz; sh++) {
      const float w = contain ? sig_contain_identity(sh, sz, kmerSize) : sig_identity(sh, sz, kmerSize);
      memcpy(&table[ani::sigstrip_entry((uint32_t)sh, (uint32_t)sz)], &w, 4);
    }
  });
  return table;
}

// a table to the device, complete on return
int sig_table_upload(ani_ctx *ctx, DevBuf &buf, const std::vector<uint32_t> &table)
{
  TRY(buf.ensure(table.size() * 4));
  HIP_TRY(hipMemcpyAsync(buf.p, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ANI_OK;
}

// Strip height: the rows of bytesPerRow each that fit kSigStripShare of what is free now, `cap` at the most; ANI_TEST_SIG_STRIP_ROWS
// (tests) replaces both.  The bounds that differ from call to call (the rows there are, a grid, a counter's width) follow at the call.
int sig_strip_rows(ani_ctx *ctx, double bytesPerRow, uint64_t cap, uint64_t *h)
{
  size_t freeB = 0, totalB = 0;
  TRY(ani_device_memory(ctx, &freeB, &totalB));
  *h = std::min<uint64_t>((uint64_t)((double)freeB * kSigStripShare / bytesPerRow), cap);
  if (const char *ev = getenv("ANI_TEST_SIG_STRIP_ROWS")) { const long long v = atoll(ev); if (v >= 1) *h = (uint64_t)v; }
  return ANI_OK;
}

// The lists of the strip's rows1 rows, which begin at row `at` of dOut / dCnt (k entries per row), into out / count: the counts through
// pinned slot 1, then the k-lists in pieces through slot 0.
int sig_lists_back(ani_ctx *ctx, const uint4 *dOut, const int32_t *dCnt, size_t at, size_t rows1, size_t k, ani_signeighbor_t *out, int32_t *count)
{
  hipStream_t st = ctx->stream;
  const size_t piece = std::max<size_t>(1, ((size_t)1 << 21) / k);               // rows per copy: 32 MiB of staging at the most
  ani_signeighbor_t *stage = nullptr; int32_t *stageCnt = nullptr;
  TRY(pinned_buffer(ctx, 0, std::min<size_t>(piece, rows1) * k * 16, (void **)&stage));
  TRY(pinned_buffer(ctx, 1, rows1 * 4, (void **)&stageCnt));
  HIP_TRY(hipMemcpyAsync(stageCnt, dCnt + at, rows1 * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(count + at, stageCnt, rows1 * 4);
  for (size_t p0 = 0; p0 < rows1; p0 += piece) {
    const size_t m = std::min<size_t>(piece, rows1 - p0) * k;
    HIP_TRY(hipMemcpyAsync(stage, dOut + (at + p0) * k, m * 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(out + (at + p0) * k, stage, m * 16);
  }
  return ANI_OK;
}

// bits of the lowest identity kept (-0.0 is 0)
uint32_t sig_min_bits(float minIdentity)
{
  const float lowest = minIdentity == 0.0f ? 0.0f : minIdentity;
  uint32_t bits; memcpy(&bits, &lowest, 4);
  return bits;
}

// checks of the C entries: the ranges of `size` and `kmerSize`, and of every length; `what` prefixes the message ("", "reference ", "query ")
int sig_check_sizes(int32_t size, int32_t kmerSize)
{
  if (size < 1 || size > kSigMaxSize) return fail(ANI_ERR_ARG, "signature size %d outside [1, %d]", size, kSigMaxSize);
  if (kmerSize < 1 || kmerSize > 16) return fail(ANI_ERR_ARG, "kmerSize %d outside [1, 16]", kmerSize);
  return ANI_OK;
}
int sig_check_lengths(const int32_t *len, int32_t n, int32_t size, const char *what)
{
  for (int32_t g = 0; g < n; g++)
    if (len[g] < 0 || len[g] > size) return fail(ANI_ERR_ARG, "%ssignature %d has length %d outside [0, %d]", what, g, len[g], size);
  return ANI_OK;
}
}  // namespace

// the merge tiles by row pitch: T x T pairs per workgroup, 2 T rows of `pitch` words in LDS
static void sigpair_launch(hipStream_t st, const uint32_t *sig, const int32_t *len, int32_t n, int32_t pitch, int32_t size, uint32_t *mat, uint64_t ld)
{
  auto tiles = [&](int t) { return dim3((unsigned)((n + t - 1) / t), (unsigned)((n + t - 1) / t)); };
  if (pitch <= 256) hipLaunchKernelGGL((k_sigpair_merge<16, 8192>), tiles(16), dim3(256), 0, st, sig, len, n, pitch, size, mat, ld);
  else if (pitch <= 1024) hipLaunchKernelGGL((k_sigpair_merge<16, kSigTileWords>), tiles(16), dim3(256), 0, st, sig, len, n, pitch, size, mat, ld);
  else if (pitch <= 2048) hipLaunchKernelGGL((k_sigpair_merge<8, kSigTileWords>), tiles(8), dim3(64), 0, st, sig, len, n, pitch, size, mat, ld);
  else hipLaunchKernelGGL((k_sigpair_merge<4, kSigTileWords>), tiles(4), dim3(64), 0, st, sig, len, n, pitch, size, mat, ld);
}

// The rows are staged and validated first, then the matrix is taken.  Device memory: the rows twice (as given and at a pitch of whole quads), 4 bytes per cell of the n x n result matrix (its upper
// triangle is used), 8 bytes per genome, 16 bytes per row returned.  Everything goes back to the pool on return.
int signature_pairs(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared,
                    ani_sigpair_t **rows, size_t *n)
{
  enum { RAW, LEN, SIG, FLAGS, MAT, CNT, OFF, OUT, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG;
  const int32_t pitch = (size + 3) & ~3;
  const uint64_t ld = (V + 3) & ~(uint64_t)3;
  uint32_t *dFlags, *dMat, *dOff; int32_t *dCnt;
  TRY(B.get(FLAGS, 64, (void **)&dFlags)); TRY(B.get(CNT, V * 4, (void **)&dCnt)); TRY(B.get(OFF, V * 4, (void **)&dOff));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  TRY(sig_stage(ctx, B.b[RAW], B.b[SIG], B.b[LEN], sig, len, V, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  const uint32_t *dSig = B.b[SIG].as<uint32_t>(); const int32_t *dLen = B.b[LEN].as<int32_t>();
  TRY(B.get(MAT, (size_t)ld * V * 4, (void **)&dMat));                 // (after the rows are known to be good: a bad row is ANI_ERR_ARG whatever the size)
  sigpair_launch(st, dSig, dLen, nG, pitch, size, dMat, ld);
  hipLaunchKernelGGL(k_sigpair_count, dim3((unsigned)nG), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, nG, minShared, dCnt);
  HIP_TRY(hipGetLastError());
  uint64_t total = 0;
  TRY(device_scan(ctx, dCnt, dOff, (uint32_t)nG, &total));
  ani_sigpair_t *out = (ani_sigpair_t *)malloc((total ? total : 1) * sizeof(ani_sigpair_t));
  if (!out) return fail(ANI_ERR_NOMEM, "host allocation of %llu pair rows failed", (unsigned long long)total);
  struct Guard { ani_sigpair_t *p; ~Guard() { free(p); } } guard{out};
  if (total) {
    uint4 *dOut;
    TRY(B.get(OUT, (size_t)total * 16, (void **)&dOut));
    hipLaunchKernelGGL(k_sigpair_write, dim3((unsigned)nG), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, nG, minShared, (const uint32_t *)dOff, dOut);
    HIP_TRY(hipGetLastError());
    // back through page-locked staging in pieces; the identities are host arithmetic (ani_abi.h)
    const size_t piece = (size_t)1 << 21;
    int32_t *stage = nullptr;
    TRY(pinned_buffer(ctx, 0, std::min<size_t>(piece, (size_t)total) * 16, (void **)&stage));
    for (size_t r0 = 0; r0 < (size_t)total; r0 += piece) {
      const size_t m = std::min<size_t>(piece, (size_t)total - r0);
      HIP_TRY(hipMemcpyAsync(stage, dOut + r0, m * 16, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const size_t step = 8192;
      parallel_for((m + step - 1) / step, (uint64_t)m * 64, [&](size_t blk) {
        for (size_t i = blk * step; i < std::min(m, (blk + 1) * step); i++) {
          const int32_t *q = stage + 4 * i;
          out[r0 + i] = ani_sigpair_t{q[0], q[1], q[2], q[3], sig_identity(q[2], q[3], kmerSize)};
        }
      });
    }
  }
  guard.p = nullptr;
  *rows = out; *n = (size_t)total;
  return ANI_OK;
}

// the strip tiles by row pitch, as sigpair_launch: rows [r0, r1), columns from r0 on
static void sigstrip_launch(hipStream_t st, const uint32_t *sig, const int32_t *len, uint32_t n, uint32_t r0, uint32_t r1, int32_t pitch, int32_t size, uint32_t *mat,
                            uint64_t ld)
{
  auto tiles = [&](uint32_t t) { return dim3((n - r0 + t - 1) / t, (r1 - r0 + t - 1) / t); };
  if (pitch <= 256) hipLaunchKernelGGL((k_sigstrip_merge<16, 8192>), tiles(16), dim3(256), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else if (pitch <= 1024) hipLaunchKernelGGL((k_sigstrip_merge<16, kSigTileWords>), tiles(16), dim3(256), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else if (pitch <= 2048) hipLaunchKernelGGL((k_sigstrip_merge<8, kSigTileWords>), tiles(8), dim3(64), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else hipLaunchKernelGGL((k_sigstrip_merge<4, kSigTileWords>), tiles(4), dim3(64), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
}

// ---- single-linkage tree of the rows plus the sketch estimates of the pairs without rows (ani_tree_single_sketch) ----
// Forest 0 is ani_tree_single's forest of the pairs with rows.  The sketch pairs then come a strip of rows at a time: the strip's cells,
// the cells that are edges (kSigStripShare of the free device memory bounds a strip: 4 bytes per cell, and 44 per edge while a strip's
// edges are sorted, as if every cell were one), the edges ranked, merged with the forest so far, and the forest stage over the two.
// Device memory: ani_tree_single's for the rows, the signatures twice while they are staged and once after, 4 s (s + 1) / 2 bytes of
// distances, 8 bytes per pair with rows, and one strip.  Nothing follows nGenomes^2.
int tree_single_sketch(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, float missingIdentity, const uint32_t *sig, const int32_t *len, int32_t size,
                       int32_t kmerSize, int32_t minShared, int32_t *children, float *height, int32_t *edges, uint8_t *source)
{
  const float dMissing = (float)(1.0 - (double)missingIdentity / 100.0);
  uint32_t dmBits; memcpy(&dmBits, &dMissing, 4);
  ctx->treeSingleRounds = 0; ctx->sigStripEdges.clear();
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG;
  const int b = id_bits(nG);
  SingleEdges forest;
  DevBuf pairKeys; uint32_t nKeys = 0;
  struct KeyGuard { DevBuf *k; ~KeyGuard() { k->release(); } } keyGuard{&pairKeys};
  TRY(single_front(ctx, rows, n, nG, dmBits, &forest, &pairKeys, &nKeys));
  TRY(single_rank(ctx, &forest, 0));
  TRY(single_forest(ctx, nG, &forest));

  // the signatures, staged and validated as for ani_signature_pairs
  enum { RAW, LEN, SIG, FLAGS, TABLE, MAT, CNT, OFF, NBUF };
  DevBufs B(NBUF);
  const int32_t pitch = (size + 3) & ~3;
  const uint64_t ld = (V + 3) & ~(uint64_t)3;
  uint32_t *dFlags, *dMat, *dOff; int32_t *dCnt;
  TRY(B.get(FLAGS, 64, (void **)&dFlags));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  TRY(sig_stage(ctx, B.b[RAW], B.b[SIG], B.b[LEN], sig, len, V, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  const uint32_t *dSig = B.b[SIG].as<uint32_t>(); const int32_t *dLen = B.b[LEN].as<int32_t>();

  if (dmBits != 0) {                                                 // (d_missing = 0: no pair lies below it)
    // bits(d) of every (shared, size'): rule 3's identity in double on the host, then ani_tree_single's rule 2
    const size_t S = (size_t)size;
    std::vector<uint32_t> table(S * (S + 1) / 2);
    parallel_for(S, (uint64_t)table.size() * 64, [&](size_t i) {
      const int32_t sz = (int32_t)i + 1;
      for (int32_t sh = 1; sh <= sz; sh++) {
        const float w = sig_identity(sh, sz, kmerSize);
        float d = (float)(1.0 - (double)w / 100.0);
        if (!(d < dMissing)) d = dMissing;
        memcpy(&table[ani::sigstrip_entry((uint32_t)sh, (uint32_t)sz)], &d, 4);
      }
    });
    TRY(sig_table_upload(ctx, B.b[TABLE], table));
    const uint32_t *dTable = B.b[TABLE].as<uint32_t>();

    // strip height: a cell and, as if every cell were an edge, the 44 bytes of an edge in its sort; the edges of a strip are numbered
    // in 32 bits
    uint64_t h;
    TRY(sig_strip_rows(ctx, 48.0 * (double)ld, 0xfffffff0ull / ld, &h));
    h = std::max<uint64_t>(1, std::min<uint64_t>(h, V - 1));
    TRY(B.get(MAT, (size_t)(h * ld) * 4, (void **)&dMat)); TRY(B.get(CNT, (size_t)h * 4, (void **)&dCnt)); TRY(B.get(OFF, (size_t)h * 4, (void **)&dOff));
    const uint64_t *realKeys = pairKeys.as<uint64_t>();
    for (uint64_t r0 = 0; r0 + 1 < V; r0 += h) {                     // (the last genome has no pair b > a)
      const uint32_t r1 = (uint32_t)std::min<uint64_t>(r0 + h, V - 1), rows1 = r1 - (uint32_t)r0;
      sigstrip_launch(st, dSig, dLen, (uint32_t)nG, (uint32_t)r0, r1, pitch, size, dMat, ld);
      hipLaunchKernelGGL(k_sigstrip_count, dim3(rows1), dim3(kTPB), 0, st, dMat, ld, (uint32_t)r0, (uint32_t)nG, minShared, (const uint32_t *)dTable, dmBits,
                         realKeys, nKeys, b, dCnt);
      HIP_TRY(hipGetLastError());
      uint64_t nE = 0;
      TRY(device_scan(ctx, dCnt, dOff, rows1, &nE));
      ctx->sigStripEdges.push_back(nE);
      if (!nE) continue;
      SingleEdges e;
      TRY(e.lo.ensure((size_t)nE * 4)); TRY(e.hi.ensure((size_t)nE * 4)); TRY(e.dKey.ensure((size_t)nE * 8)); TRY(e.idx.ensure((size_t)nE * 4));
      uint32_t *eLo = e.lo.as<uint32_t>(), *eHi = e.hi.as<uint32_t>(), *idx = e.idx.as<uint32_t>(); uint64_t *dKey = e.dKey.as<uint64_t>();
      hipLaunchKernelGGL(k_sigstrip_write, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, (uint32_t)nG, (const uint32_t *)dOff,
                         eLo, eHi, dKey, idx);
      HIP_TRY(hipGetLastError());
      e.n = (uint32_t)nE;
      TRY(single_rank(ctx, &e, 1));
      TRY(single_merge(ctx, &forest, &e));
      TRY(single_forest(ctx, nG, &forest));
    }
  }
  return single_finish(ctx, forest, nG, dMissing, children, height, edges, source);
}

// ---- nearest neighbours under the sketch estimate (ani_signature_neighbors) ----
// the rectangular tiles by row pitch, as sigpair_launch: rows [r0, r1), all columns
static void signeigh_launch(hipStream_t st, const uint32_t *sig, const int32_t *len, uint32_t n, uint32_t r0, uint32_t r1, int32_t pitch, int32_t size, uint32_t *mat,
                            uint64_t ld)
{
  auto tiles = [&](uint32_t t) { return dim3((n + t - 1) / t, (r1 - r0 + t - 1) / t); };
  if (pitch <= 256) hipLaunchKernelGGL((k_signeigh_merge<16, 8192>), tiles(16), dim3(256), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else if (pitch <= 1024) hipLaunchKernelGGL((k_signeigh_merge<16, kSigTileWords>), tiles(16), dim3(256), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else if (pitch <= 2048) hipLaunchKernelGGL((k_signeigh_merge<8, kSigTileWords>), tiles(8), dim3(64), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
  else hipLaunchKernelGGL((k_signeigh_merge<4, kSigTileWords>), tiles(4), dim3(64), 0, st, sig, len, n, r0, r1, pitch, size, mat, ld);
}

// The signatures are staged and validated as for ani_signature_pairs, the identity bits of every (shared, size') come from the host, and
// the rows of the range go through the device a strip at a time: the strip's cells against every genome, then the k nearest of each row,
// written into the row's place of the range's output and copied back through page-locked staging.  Every pair is merged once from
// each of its ends.  Device memory: the signatures twice while they are staged and once after, 2 s (s + 1) bytes of identities,
// 16 k + 4 bytes per row of the range, and one strip (kSigStripShare of what is free then, 4 bytes per cell).  Nothing follows nGenomes^2.
int signature_neighbors(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity,
                        int32_t k, int32_t rowBegin, int32_t rowEnd, ani_signeighbor_t *out, int32_t *count)
{
  enum { RAW, LEN, SIG, FLAGS, TABLE, MAT, OUT, CNT, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG, R = (size_t)(rowEnd - rowBegin);
  const int32_t pitch = (size + 3) & ~3;
  const uint64_t ld = (V + 3) & ~(uint64_t)3;
  uint32_t *dFlags, *dMat; int32_t *dCnt; uint4 *dOut;
  TRY(B.get(FLAGS, 64, (void **)&dFlags));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  TRY(sig_stage(ctx, B.b[RAW], B.b[SIG], B.b[LEN], sig, len, V, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  const uint32_t *dSig = B.b[SIG].as<uint32_t>(); const int32_t *dLen = B.b[LEN].as<int32_t>();

  TRY(sig_table_upload(ctx, B.b[TABLE], sig_identity_table(size, kmerSize, false)));
  const uint32_t *dTable = B.b[TABLE].as<uint32_t>();
  const uint32_t minBits = sig_min_bits(minIdentity);

  TRY(B.get(OUT, R * (size_t)k * 16, (void **)&dOut)); TRY(B.get(CNT, R * 4, (void **)&dCnt));
  // strip height: 4 bytes per cell; the grid of the 4 x 4 tiles bounds it too
  uint64_t h;
  TRY(sig_strip_rows(ctx, 4.0 * (double)ld, kNoStripCap, &h));
  h = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(h, R), 4 * 65535));
  TRY(B.get(MAT, (size_t)(h * ld) * 4, (void **)&dMat));
  for (uint64_t r0 = (uint64_t)rowBegin; r0 < (uint64_t)rowEnd; r0 += h) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(r0 + h, (uint64_t)rowEnd), rows1 = r1 - (uint32_t)r0;
    const size_t at = (size_t)(r0 - (uint64_t)rowBegin);
    signeigh_launch(st, dSig, dLen, (uint32_t)nG, (uint32_t)r0, r1, pitch, size, dMat, ld);
    hipLaunchKernelGGL(k_signeigh_select, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, (uint32_t)rowBegin, (uint32_t)nG, minShared,
                       (const uint32_t *)dTable, minBits, k, dOut, dCnt);
    HIP_TRY(hipGetLastError());
    ctx->sigNeighStrips++;
    TRY(sig_lists_back(ctx, dOut, dCnt, at, rows1, (size_t)k, out, count));
  }
  return ANI_OK;
}

// ---- the nearest references of every query under the sketch estimate (ani_signature_screen) ----
// The tile by strip height and row pitch.  A strip of at least T queries, T the edge of the pair tiles at this pitch, takes the square
// tile; a lower one the thin tile of one query and 64 references, whose LDS is the query row alone.  ANI_TEST_SIG_SCREEN_SHAPE = square or
// thin (tests, tools/sketch_probe.py) forces a shape.  shape[0 .. 2) = TQ, TR of the tile taken.  mode < 0: the Mash merge of
// k_sigscreen_merge; otherwise the containment walk of k_sigcontain_merge in that mode, in the same shapes, the
// square tiles with kSigContainPad more words of LDS for their row pitch there.
static void sigscreen_launch(hipStream_t st, const uint32_t *refSig, const int32_t *refLen, uint32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, uint32_t q0,
                             uint32_t q1, int32_t pitch, int32_t size, int32_t mode, uint32_t *mat, uint64_t ld, int32_t *shape)
{
  const uint32_t T = pitch <= 1024 ? 16u : pitch <= 2048 ? 8u : 4u;
  bool thin = q1 - q0 < T;
  if (const char *ev = getenv("ANI_TEST_SIG_SCREEN_SHAPE")) { if (!strcmp(ev, "square")) thin = false; else if (!strcmp(ev, "thin")) thin = true; }
  auto tiles = [&](uint32_t tq, uint32_t tr) { return dim3((nRef + tr - 1) / tr, (q1 - q0 + tq - 1) / tq); };
#define ANI_SCREEN(TQ, TR, WORDS, LANES) do { \
    if (mode < 0) hipLaunchKernelGGL((k_sigscreen_merge<TQ, TR, WORDS>), tiles(TQ, TR), dim3(LANES), 0, st, refSig, refLen, nRef, qrySig, qryLen, q0, q1, pitch, size, \
                                     mat, ld); \
    else hipLaunchKernelGGL((k_sigcontain_merge<TQ, TR, (TQ > 1 ? WORDS + kSigContainPad : WORDS)>), tiles(TQ, TR), dim3(LANES), 0, st, refSig, refLen, nRef, qrySig, \
                            qryLen, q0, q1, pitch, size, mode, mat, ld); } while (0)
  if (thin) {
    if (pitch <= 1024) ANI_SCREEN(1, kSigScreenThinRefs, 1024, 64);
    else ANI_SCREEN(1, kSigScreenThinRefs, kSigMaxSize, 64);
  }
  else if (pitch <= 256) ANI_SCREEN(16, 16, 8192, 256);
  else if (pitch <= 1024) ANI_SCREEN(16, 16, kSigTileWords, 256);
  else if (pitch <= 2048) ANI_SCREEN(8, 8, kSigTileWords, 64);
  else ANI_SCREEN(4, 4, kSigTileWords, 64);
#undef ANI_SCREEN
  shape[0] = thin ? 1 : (int32_t)T; shape[1] = thin ? kSigScreenThinRefs : (int32_t)T;
}

// Both sets are staged and validated as for ani_signature_pairs, the references once; the identity bits of every (shared, size') come
// from the host; the queries go through the device a strip at a time: the strip's cells against every reference, then the k nearest of
// each query, written into the query's place of the output and copied back through page-locked staging.  Device memory: either set
// twice while it is staged and once after, 2 s (s + 1) bytes of identities, 16 k + 4 bytes per query, and one strip (kSigStripShare of
// what is free then, 4 bytes per cell).  Nothing follows nRef * nQry.
// Shared by the two estimates: mode < 0 is ani_signature_screen (the Mash merge and its identity table), mode 0 .. 2 is
// ani_signature_screen_contain (the containment walk in that mode and the containment table); everything else is the same code.
static int screen_run(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                      int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, int32_t mode, ani_signeighbor_t *out, int32_t *count)
{
  enum { RRAW, RLEN, RSIG, QRAW, QLEN, QSIG, FLAGS, TABLE, MAT, OUT, CNT, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t R = (size_t)nRef, Q = (size_t)nQry;
  const int32_t pitch = (size + 3) & ~3;
  const uint64_t ld = (R + 3) & ~(uint64_t)3;
  uint32_t *dFlags, *dMat; int32_t *dCnt; uint4 *dOut;
  TRY(B.get(FLAGS, 64, (void **)&dFlags));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  if (R) { TRY(sig_stage(ctx, B.b[RRAW], B.b[RSIG], B.b[RLEN], refSig, refLen, R, size, pitch, dFlags)); }
  TRY(sig_stage(ctx, B.b[QRAW], B.b[QSIG], B.b[QLEN], qrySig, qryLen, Q, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  if (!R) {                                                            // no references: every list is empty
    for (size_t i = 0; i < Q * (size_t)k; i++) out[i] = ani_signeighbor_t{-1, 0, 0, 0.0f};
    std::fill(count, count + Q, 0);
    return ANI_OK;
  }
  const uint32_t *dRefSig = B.b[RSIG].as<uint32_t>(), *dQrySig = B.b[QSIG].as<uint32_t>();
  const int32_t *dRefLen = B.b[RLEN].as<int32_t>(), *dQryLen = B.b[QLEN].as<int32_t>();

  TRY(sig_table_upload(ctx, B.b[TABLE], sig_identity_table(size, kmerSize, mode >= 0)));
  const uint32_t *dTable = B.b[TABLE].as<uint32_t>();
  const uint32_t minBits = sig_min_bits(minIdentity);

  TRY(B.get(OUT, Q * (size_t)k * 16, (void **)&dOut)); TRY(B.get(CNT, Q * 4, (void **)&dCnt));
  // strip height: 4 bytes per cell; the grid of the 4 x 4 tiles bounds it too
  uint64_t h;
  TRY(sig_strip_rows(ctx, 4.0 * (double)ld, kNoStripCap, &h));
  h = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(h, Q), 65535));
  TRY(B.get(MAT, (size_t)(h * ld) * 4, (void **)&dMat));
  for (uint64_t q0 = 0; q0 < Q; q0 += h) {
    const uint32_t q1 = (uint32_t)std::min<uint64_t>(q0 + h, Q), rows1 = q1 - (uint32_t)q0;
    sigscreen_launch(st, dRefSig, dRefLen, (uint32_t)nRef, dQrySig, dQryLen, (uint32_t)q0, q1, pitch, size, mode, dMat, ld, ctx->sigScreenTile);
    hipLaunchKernelGGL(k_sigscreen_select, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)q0, (uint32_t)nRef, minShared,
                       (const uint32_t *)dTable, minBits, k, dOut, dCnt);
    HIP_TRY(hipGetLastError());
    ctx->sigScreenStrips++;
    TRY(sig_lists_back(ctx, dOut, dCnt, (size_t)q0, rows1, (size_t)k, out, count));
  }
  return ANI_OK;
}

int signature_screen(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                     int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, ani_signeighbor_t *out, int32_t *count)
{
  return screen_run(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, -1, out, count);
}

// ---- the same under the containment estimate (ani_signature_screen_contain) ----
int signature_screen_contain(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                             int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, int32_t mode, ani_signeighbor_t *out, int32_t *count)
{
  return screen_run(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, mode, out, count);
}

// ---- the pair graph under either sketch estimate, streamed (ani_signature_graph) ----
// The signatures are staged and validated as for ani_signature_neighbors and the identity bits of every (shared, size-or-d) come from
// the host.  The rows of the range go through the device a strip at a time: the strip's cells right of the diagonal (the triangular
// Mash tiles of k_sigstrip_merge, or the containment walk in mode MAX with the strip as the queries and the genomes from r0 on as the
// references, its cell pointer moved r0 columns so that both leave cell (a, b) at row a - r0, column b), the kept cells of every row
// counted and scanned, then written as records behind the row's offset and copied back through page-locked staging.  The host does no
// arithmetic on them.  Device memory: the signatures twice while they are staged and once after, 2 s (s + 1) bytes of identities, one
// strip (kSigStripShare of what is free then, at 24 bytes per cell: the cell and, as if every cell were kept, its record) with 8 bytes
// per row, 20 bytes per kept pair of the strip.  Host: 20 bytes per kept pair of the range.  Nothing follows nGenomes^2.
// A strip holds at most kSigGraphMaxPairs cells (a forced height included), so the 32-bit sums of its kept cells are exact.
constexpr uint64_t kSigGraphMaxPairs = 0xfffffff0ull;

int signature_graph(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity,
                    int32_t estimate, int32_t rowBegin, int32_t rowEnd, ani_sigpair_t **rows, size_t *n)
{
  enum { RAW, LEN, SIG, FLAGS, TABLE, MAT, CNT, OFF, OUT, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG, R = (size_t)(rowEnd - rowBegin);
  const int32_t pitch = (size + 3) & ~3;
  const uint64_t ld = (V + 3) & ~(uint64_t)3;
  uint32_t *dFlags, *dMat, *dOff, *dOut; int32_t *dCnt;
  TRY(B.get(FLAGS, 64, (void **)&dFlags));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  TRY(sig_stage(ctx, B.b[RAW], B.b[SIG], B.b[LEN], sig, len, V, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  const uint32_t *dSig = B.b[SIG].as<uint32_t>(); const int32_t *dLen = B.b[LEN].as<int32_t>();

  const bool contain = estimate == ANI_GRAPH_CONTAIN_MAX;
  TRY(sig_table_upload(ctx, B.b[TABLE], sig_identity_table(size, kmerSize, contain)));
  const uint32_t *dTable = B.b[TABLE].as<uint32_t>();
  const uint32_t minBits = sig_min_bits(minIdentity);

  // strip height: a cell and, as if every cell were kept, its record; the grid of the thin tile (one row of queries per workgroup)
  // bounds it too, and so do the 32 bits in which device_scan sums the kept cells of a strip: a strip of at most 2^32 - 16 cells cannot
  // wrap them, whatever is kept, so the limit check below sees every strip's true count
  uint64_t h;
  TRY(sig_strip_rows(ctx, 24.0 * (double)ld, kNoStripCap, &h));
  h = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(h, R), 65535), kSigGraphMaxPairs / ld));
  TRY(B.get(MAT, (size_t)(h * ld) * 4, (void **)&dMat)); TRY(B.get(CNT, (size_t)h * 4, (void **)&dCnt)); TRY(B.get(OFF, (size_t)h * 4, (void **)&dOff));

  const size_t piece = (size_t)1 << 20;                                // records per copy: 20 MiB of staging
  ani_sigpair_t *stage = nullptr;
  ani_sigpair_t *out = nullptr;
  size_t have = 0, cap = 0;
  struct Guard { ani_sigpair_t **p; ~Guard() { free(*p); } } guard{&out};
  for (uint64_t r0 = (uint64_t)rowBegin; r0 < (uint64_t)rowEnd; r0 += h) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(r0 + h, (uint64_t)rowEnd), rows1 = r1 - (uint32_t)r0;
    if (contain) {
      int32_t shape[2];
      sigscreen_launch(st, dSig + (size_t)r0 * (size_t)pitch, dLen + r0, (uint32_t)(V - r0), dSig, dLen, (uint32_t)r0, r1, pitch, size, ANI_CONTAIN_MAX,
                       dMat + r0, ld, shape);
    }
    else sigstrip_launch(st, dSig, dLen, (uint32_t)nG, (uint32_t)r0, r1, pitch, size, dMat, ld);
    hipLaunchKernelGGL(k_siggraph_count, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, (uint32_t)nG, minShared,
                       (const uint32_t *)dTable, minBits, dCnt);
    HIP_TRY(hipGetLastError());
    ctx->sigGraphStrips++;
    uint64_t nE = 0;
    TRY(device_scan(ctx, dCnt, dOff, rows1, &nE, kSigGraphMaxPairs));
    if ((uint64_t)have + nE > kSigGraphMaxPairs)                       // (before anything of the strip is written)
      return fail(ANI_ERR_LIMIT, "more than %llu kept pairs in rows [%d, %d): split the range", (unsigned long long)kSigGraphMaxPairs, rowBegin, rowEnd);
    if (!nE) continue;
    if (have + (size_t)nE > cap) {
      const size_t want = std::max<size_t>(have + (size_t)nE, cap + cap / 2);
      ani_sigpair_t *grown = (ani_sigpair_t *)realloc(out, want * sizeof(ani_sigpair_t));
      if (!grown) return fail(ANI_ERR_NOMEM, "host allocation of %llu pair rows failed", (unsigned long long)want);
      out = grown; cap = want;
    }
    TRY(B.get(OUT, (size_t)nE * sizeof(ani_sigpair_t), (void **)&dOut));
    hipLaunchKernelGGL(k_siggraph_write, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, (uint32_t)nG, minShared,
                       (const uint32_t *)dTable, minBits, (const uint32_t *)dOff, dOut);
    HIP_TRY(hipGetLastError());
    TRY(pinned_buffer(ctx, 0, std::min<size_t>(piece, (size_t)nE) * sizeof(ani_sigpair_t), (void **)&stage));
    for (size_t p0 = 0; p0 < (size_t)nE; p0 += piece) {
      const size_t m = std::min<size_t>(piece, (size_t)nE - p0);
      HIP_TRY(hipMemcpyAsync(stage, dOut + p0 * kSigGraphRecordWords, m * sizeof(ani_sigpair_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      memcpy(out + have + p0, stage, m * sizeof(ani_sigpair_t));
    }
    have += (size_t)nE;
  }
  *rows = out; *n = have;
  out = nullptr;
  return ANI_OK;
}

// ---- greedy representative clustering under the sketch estimate (ani_signature_cluster) ----
// Strip height at the most, by genome count: the strip's own rows x rows block is merged whether greedy clustering needs its pairs or
// not, so the blocks together (n h cells) stay at a sixteenth of the n^2 / 2 pairs of the composition, within [256, 4096] rows: below
// 256 the resolve workgroup's lanes idle and the launches of a strip outweigh its cells, above kSigClusterMaxStrip the covered words
// of a strip do not fit the LDS the resolve kernel declares.
static uint64_t sigcluster_strip_cap(uint64_t n) { return std::min<uint64_t>(std::max<uint64_t>(n / 32, 256), (uint64_t)kSigClusterMaxStrip); }

// The strip's own rows x rows block under the containment estimate in mode MAX, from its upper triangle (k_sigcontain_tri, DESIGN.md
// section 2.22): the square tile of the row pitch at every strip height.  A strip lower than the tile is one diagonal tile, which stages
// the strip's rows once, so the thin tile of sigscreen_launch has nothing to save here and ANI_TEST_SIG_SCREEN_SHAPE does not act.
static void sigcontain_tri_launch(hipStream_t st, const uint32_t *sig, const int32_t *len, uint32_t h, int32_t pitch, int32_t size, uint32_t *mat, uint64_t ld)
{
  auto tiles = [&](uint32_t t) { const uint32_t n = (h + t - 1) / t; return dim3(n * (n + 1) / 2); };
  if (pitch <= 256) hipLaunchKernelGGL((k_sigcontain_tri<16, 8192 + kSigContainPad>), tiles(16), dim3(256), 0, st, sig, len, h, pitch, size, mat, ld);
  else if (pitch <= 1024) hipLaunchKernelGGL((k_sigcontain_tri<16, kSigTileWords + kSigContainPad>), tiles(16), dim3(256), 0, st, sig, len, h, pitch, size, mat, ld);
  else if (pitch <= 2048) hipLaunchKernelGGL((k_sigcontain_tri<8, kSigTileWords + kSigContainPad>), tiles(8), dim3(64), 0, st, sig, len, h, pitch, size, mat, ld);
  else hipLaunchKernelGGL((k_sigcontain_tri<4, kSigTileWords + kSigContainPad>), tiles(4), dim3(64), 0, st, sig, len, h, pitch, size, mat, ld);
}

// The signatures are staged and validated as for ani_signature_pairs and the identity bits of every (shared, size') come from the host.
// First sweep, strips in id order: the strip against the representatives found before it (k_sigscreen_merge with the representatives'
// rows as the references, then k_sigcluster_best), the strip against itself and k_sigcluster_resolve, which names the strip's
// representatives; k_sigcluster_gather appends their rows.  Second sweep: the members of every strip against the representatives found
// after it.  Every (genome, representative) pair is merged once, and besides them only the pairs inside a strip.  The host waits once
// per strip of the first sweep, for the count of representatives, which sizes the next launches.  Device memory: the signatures twice
// while they are staged and once after, the representatives' rows (room for every genome: one more copy at the most), 2 s (s + 1) bytes
// of identities, 28 bytes per genome, and one strip of rows x max(representatives, rows) 4-byte cells.  Nothing follows nGenomes^2.
// Shared by the two estimates: mode < 0 is ani_signature_cluster (the Mash merge and its identity table); mode ANI_CONTAIN_MAX is
// ani_signature_cluster_contain: the containment walk in the rectangular launches, the containment table, and the
// strip's own block from its upper triangle, whose cells are symmetric in that mode, unless ANI_TEST_SIG_CLUSTER_TRI = 0 (tests,
// tools/sketch_probe.py) sends it through the full rows x rows launch as well.  stats[2] counts the cells walked: rows (rows - 1) / 2 for
// a triangular launch.
static int cluster_run(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity,
                       int32_t mode, int32_t *representative, ani_signeighbor_t *link)
{
  enum { RAW, LEN, SIG, FLAGS, TABLE, REPSIG, REPLEN, REPID, REPCNT, BEST, CELL, MEMLEN, MAT, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG;
  const int32_t pitch = (size + 3) & ~3;
  auto quads = [](uint64_t x) { return (x + 3) & ~(uint64_t)3; };
  uint32_t *dFlags, *dRepSig, *dRepId, *dRepCnt, *dCell, *dMat; int32_t *dRepLen, *dMemLen; uint64_t *dBest;
  TRY(B.get(FLAGS, 64, (void **)&dFlags));
  HIP_TRY(hipMemsetAsync(dFlags, 0, 64, st));
  TRY(sig_stage(ctx, B.b[RAW], B.b[SIG], B.b[LEN], sig, len, V, size, pitch, dFlags));
  TRY(sig_stage_check(ctx, dFlags));
  const uint32_t *dSig = B.b[SIG].as<uint32_t>(); const int32_t *dLen = B.b[LEN].as<int32_t>();
  uint32_t *host = nullptr;                                            // (the count of representatives after a strip)
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));

  TRY(sig_table_upload(ctx, B.b[TABLE], sig_identity_table(size, kmerSize, mode >= 0)));
  const uint32_t *dTable = B.b[TABLE].as<uint32_t>();
  uint32_t minBits; memcpy(&minBits, &minIdentity, 4);                 // (> 0: a running best of 0 is "no edge")
  bool tri = mode >= 0;
  if (const char *ev = getenv("ANI_TEST_SIG_CLUSTER_TRI")) { if (!strcmp(ev, "0")) tri = false; }

  TRY(B.get(REPSIG, V * (size_t)pitch * 4, (void **)&dRepSig)); TRY(B.get(REPLEN, V * 4, (void **)&dRepLen)); TRY(B.get(REPID, V * 4, (void **)&dRepId));
  TRY(B.get(REPCNT, 64, (void **)&dRepCnt)); TRY(B.get(BEST, V * 8, (void **)&dBest)); TRY(B.get(CELL, V * 4, (void **)&dCell));
  TRY(B.get(MEMLEN, V * 4, (void **)&dMemLen));
  HIP_TRY(hipMemsetAsync(dBest, 0, V * 8, st)); HIP_TRY(hipMemsetAsync(dCell, 0, V * 4, st));
  // strip height: 4 bytes per cell of a strip against every genome (all of them may be representatives), and the cap by genome count
  uint64_t h;
  TRY(sig_strip_rows(ctx, 4.0 * (double)quads(V), sigcluster_strip_cap(V), &h));
  h = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(h, V), (uint64_t)kSigClusterMaxStrip));
  uint64_t *stats = ctx->sigClusterStats;
  int32_t shape[2];

  // first sweep.  repAt[s]: the representatives after strip s; members[s]: its rows that are none
  std::vector<uint32_t> repAt, members;
  uint32_t nRep = 0;
  for (uint64_t r0 = 0; r0 < V; r0 += h) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(r0 + h, V), rows1 = r1 - (uint32_t)r0;
    // (the stream is idle here: the buffer may move.  Twice the representatives, so that it moves a logarithmic number of times)
    TRY(B.get(MAT, (size_t)rows1 * (size_t)quads(std::max<uint64_t>(std::min<uint64_t>(2 * (uint64_t)nRep, V), h)) * 4, (void **)&dMat));
    if (nRep) {
      const uint64_t ld = quads(nRep);
      sigscreen_launch(st, dRepSig, dRepLen, nRep, dSig, dLen, (uint32_t)r0, r1, pitch, size, mode, dMat, ld, shape);
      hipLaunchKernelGGL(k_sigcluster_best, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, nRep, (const uint32_t *)dRepId, minShared,
                         (const uint32_t *)dTable, minBits, dBest, dCell);
      stats[2] += (uint64_t)rows1 * nRep;
    }
    const uint64_t ld = quads(rows1);
    if (tri) sigcontain_tri_launch(st, dSig + (size_t)r0 * (size_t)pitch, dLen + r0, rows1, pitch, size, dMat, ld);
    else sigscreen_launch(st, dSig + (size_t)r0 * (size_t)pitch, dLen + r0, rows1, dSig, dLen, (uint32_t)r0, r1, pitch, size, mode, dMat, ld, shape);
    hipLaunchKernelGGL(k_sigcluster_resolve, dim3(1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, rows1, nRep, minShared, (const uint32_t *)dTable,
                       minBits, (const int32_t *)dLen, dBest, dCell, dMemLen, dRepId, dRepCnt);
    HIP_TRY(hipGetLastError());
    stats[2] += tri ? (uint64_t)rows1 * (rows1 - 1) / 2 : (uint64_t)rows1 * rows1;
    HIP_TRY(hipMemcpyAsync(host, dRepCnt, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t found = host[0] - nRep;
    if (found) {
      hipLaunchKernelGGL(k_sigcluster_gather, dim3(found), dim3(kTPB), 0, st, (const uint32_t *)dSig, (const int32_t *)dLen, (const uint32_t *)dRepId, nRep, pitch,
                         dRepSig, dRepLen);
      HIP_TRY(hipGetLastError());
    }
    stats[3] += (uint64_t)found * ((rows1 + kTPB - 1) / kTPB);
    nRep += found;
    repAt.push_back(nRep); members.push_back(rows1 - found);
    stats[0]++;
  }
  stats[1] = nRep;

  // second sweep: the members of a strip against the representatives found after it (a representative's length is 0 in dMemLen)
  uint64_t cells = 0;
  for (size_t s = 0; s < repAt.size(); s++)
    if (members[s]) cells = std::max<uint64_t>(cells, std::min<uint64_t>(h, V - s * h) * quads(nRep - repAt[s]));
  HIP_TRY(hipStreamSynchronize(st));                                   // (the last gather; the buffer may move)
  if (cells) { TRY(B.get(MAT, (size_t)cells * 4, (void **)&dMat)); }
  for (size_t s = 0; s < repAt.size(); s++) {
    const uint32_t later = nRep - repAt[s];
    if (!later || !members[s]) continue;
    const uint64_t r0 = s * h, ld = quads(later);
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(r0 + h, V), rows1 = r1 - (uint32_t)r0;
    sigscreen_launch(st, dRepSig + (size_t)repAt[s] * (size_t)pitch, dRepLen + repAt[s], later, dSig, dMemLen, (uint32_t)r0, r1, pitch, size, mode, dMat, ld, shape);
    hipLaunchKernelGGL(k_sigcluster_best, dim3(rows1), dim3(kTPB), 0, st, (const uint32_t *)dMat, ld, (uint32_t)r0, later, (const uint32_t *)dRepId + repAt[s],
                       minShared, (const uint32_t *)dTable, minBits, dBest, dCell);
    HIP_TRY(hipGetLastError());
    stats[2] += (uint64_t)rows1 * later;
  }

  // the keys back, decoded on the host; the identities are host arithmetic (ani_abi.h)
  std::vector<uint64_t> best(V); std::vector<uint32_t> cell(V);
  HIP_TRY(hipMemcpyAsync(best.data(), dBest, V * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cell.data(), dCell, V * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const size_t step = 8192;
  parallel_for((V + step - 1) / step, (uint64_t)V * 64, [&](size_t blk) {
    for (size_t i = blk * step; i < std::min(V, (blk + 1) * step); i++) {
      if (!best[i]) { representative[i] = (int32_t)i; link[i] = ani_signeighbor_t{-1, 0, 0, 0.0f}; continue; }
      const int32_t rep = (int32_t)(0xffffffffu - (uint32_t)best[i]), sh = (int32_t)(cell[i] >> 16), sz = (int32_t)(cell[i] & 0xffffu);
      representative[i] = rep;
      link[i] = ani_signeighbor_t{rep, sh, sz, mode < 0 ? sig_identity(sh, sz, kmerSize) : sig_contain_identity(sh, sz, kmerSize)};
    }
  });
  return ANI_OK;
}

int signature_cluster(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity,
                      int32_t *representative, ani_signeighbor_t *link)
{
  return cluster_run(ctx, sig, len, nG, size, kmerSize, minShared, minIdentity, -1, representative, link);
}

// ---- the same under the containment estimate (ani_signature_cluster_contain) ----
int signature_cluster_contain(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nG, int32_t size, int32_t kmerSize, int32_t minShared,
                              float minIdentity, int32_t mode, int32_t *representative, ani_signeighbor_t *link)
{
  return cluster_run(ctx, sig, len, nG, size, kmerSize, minShared, minIdentity, mode, representative, link);
}

}  // namespace anih

extern "C" {

int ani_tree_single_sketch(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity, const uint32_t *sig, const int32_t *len,
                           int32_t size, int32_t kmerSize, int32_t minShared, int32_t *children, float *height, int32_t *edges, uint8_t *source)
{
  if (!ctx || (n && !rows) || (nGenomes > 1 && (!children || !height || !sig || !len))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  if (!(missingIdentity >= 0.0f && missingIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "missingIdentity %g outside [0, 100]", (double)missingIdentity);
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 1) return fail(ANI_ERR_ARG, "minShared %d below 1", minShared);
  if (nGenomes > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d genomes: the cluster ids of the tree take at most 2^30", nGenomes);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  if (nGenomes <= 1) return ANI_OK;
  TRY(sig_check_lengths(len, nGenomes, size, ""));
  HIP_TRY(hipSetDevice(ctx->device));
  try { return tree_single_sketch(ctx, rows, n, nGenomes, missingIdentity, sig, len, size, kmerSize, minShared, children, height, edges, source); }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_tree_single_sketch_strips(const ani_ctx *ctx, uint64_t *edgesPerStrip, size_t cap)
{
  if (!ctx) return 0;
  for (size_t i = 0; i < ctx->sigStripEdges.size() && i < cap && edgesPerStrip; i++) edgesPerStrip[i] = ctx->sigStripEdges[i];
  return (int)ctx->sigStripEdges.size();
}

int ani_sketch_signatures(const ani_sketch *sk, int32_t size, uint32_t *sig, int32_t *len)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (size < 1 || size > kSigMaxSize) return fail(ANI_ERR_ARG, "signature size %d outside [1, %d]", size, kSigMaxSize);
  if (sk->nGenomes > 0 && (!sig || !len)) return fail(ANI_ERR_ARG, "null argument");
  if (sk->nGenomes <= 0) return ANI_OK;
  HIP_TRY(hipSetDevice(sk->device));
  return sketch_signatures(sk, size, sig, len);
}

int ani_signature_pairs(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                        ani_sigpair_t **rows, size_t *n)
{
  if (!ctx || !rows || !n || (nGenomes > 0 && (!sig || !len))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 0) return fail(ANI_ERR_ARG, "negative minShared");
  if (nGenomes > 65536) return fail(ANI_ERR_LIMIT, "%d genomes: the pair step takes at most 65536", nGenomes);
  TRY(sig_check_lengths(len, nGenomes, size, ""));
  if (nGenomes <= 1) {                                                 // nothing to compare; a lone row is still checked
    for (int32_t r = 1; nGenomes == 1 && r < len[0]; r++)
      if (sig[r - 1] >= sig[r]) return fail(ANI_ERR_ARG, "a signature does not ascend strictly");
    *rows = (ani_sigpair_t *)malloc(sizeof(ani_sigpair_t)); *n = 0;
    return *rows ? ANI_OK : fail(ANI_ERR_NOMEM, "host allocation failed");
  }
  HIP_TRY(hipSetDevice(ctx->device));
  return signature_pairs(ctx, sig, len, nGenomes, size, kmerSize, minShared, rows, n);
}


int ani_signature_neighbors(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                            float minIdentity, int32_t k, int32_t rowBegin, int32_t rowEnd, ani_signeighbor_t *out, int32_t *count)
{
  if (!ctx) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 1) return fail(ANI_ERR_ARG, "minShared %d below 1", minShared);
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (k < 1 || k > ani::kSigNeighMaxK) return fail(ANI_ERR_ARG, "k %d outside [1, %d]", k, ani::kSigNeighMaxK);
  if (nGenomes > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d genomes: the neighbour lists take at most 2^30", nGenomes);
  if (rowBegin < 0 || rowBegin > rowEnd || rowEnd > nGenomes) return fail(ANI_ERR_ARG, "rows [%d, %d) outside [0, %d]", rowBegin, rowEnd, nGenomes);
  ctx->sigNeighStrips = 0;
  if (nGenomes == 0 || rowBegin == rowEnd) return ANI_OK;
  if (!sig || !len || !out || !count) return fail(ANI_ERR_ARG, "null argument");
  TRY(sig_check_lengths(len, nGenomes, size, ""));
  HIP_TRY(hipSetDevice(ctx->device));
  try { return signature_neighbors(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, k, rowBegin, rowEnd, out, count); }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_signature_neighbors_strips(const ani_ctx *ctx) { return ctx ? ctx->sigNeighStrips : 0; }

int ani_signature_graph(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                        float minIdentity, int32_t estimate, int32_t rowBegin, int32_t rowEnd, ani_sigpair_t **rows, size_t *n)
{
  if (!ctx || !rows || !n) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 1) return fail(ANI_ERR_ARG, "minShared %d below 1", minShared);
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (estimate < ANI_GRAPH_MASH || estimate > ANI_GRAPH_CONTAIN_MAX) return fail(ANI_ERR_ARG, "estimate %d outside [0, 1]", estimate);
  if (nGenomes > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d genomes: the pair graph takes at most 2^30", nGenomes);
  if (rowBegin < 0 || rowBegin > rowEnd || rowEnd > nGenomes) return fail(ANI_ERR_ARG, "rows [%d, %d) outside [0, %d]", rowBegin, rowEnd, nGenomes);
  ctx->sigGraphStrips = 0;
  *rows = nullptr; *n = 0;
  if (nGenomes <= 1 || rowBegin == rowEnd) return ANI_OK;
  if (!sig || !len) return fail(ANI_ERR_ARG, "null argument");
  TRY(sig_check_lengths(len, nGenomes, size, ""));
  HIP_TRY(hipSetDevice(ctx->device));
  try { return signature_graph(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, estimate, rowBegin, rowEnd, rows, n); }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_signature_graph_strips(const ani_ctx *ctx) { return ctx ? ctx->sigGraphStrips : 0; }

// the two screen calls: the checks of ani_signature_screen's rules 4 - 6 and, with `contain`, of ani_signature_screen_contain's rule 7,
// then the call; without `contain` it is ani_signature_screen and the mode plays no part
static int screen_entry(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                        int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, bool contain, int32_t mode, ani_signeighbor_t *out,
                        int32_t *count)
{
  if (!ctx) return fail(ANI_ERR_ARG, "null argument");
  if (nRef < 0 || nQry < 0) return fail(ANI_ERR_ARG, "negative genome count");
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 1) return fail(ANI_ERR_ARG, "minShared %d below 1", minShared);
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (k < 1 || k > ani::kSigNeighMaxK) return fail(ANI_ERR_ARG, "k %d outside [1, %d]", k, ani::kSigNeighMaxK);
  if (contain && (mode < ANI_CONTAIN_QUERY || mode > ANI_CONTAIN_MAX)) return fail(ANI_ERR_ARG, "containment mode %d outside [0, 2]", mode);
  if (nRef > (1 << 30) || nQry > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d references, %d queries: the screen takes at most 2^30 of either", nRef, nQry);
  ctx->sigScreenStrips = 0; ctx->sigScreenTile[0] = ctx->sigScreenTile[1] = 0;
  if (nQry == 0) return ANI_OK;
  if (!qrySig || !qryLen || !out || !count || (nRef > 0 && (!refSig || !refLen))) return fail(ANI_ERR_ARG, "null argument");
  TRY(sig_check_lengths(refLen, nRef, size, "reference "));
  TRY(sig_check_lengths(qryLen, nQry, size, "query "));
  HIP_TRY(hipSetDevice(ctx->device));
  try {
    if (contain) return signature_screen_contain(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, mode, out, count);
    return signature_screen(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, out, count);
  }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_signature_screen(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen, int32_t nQry,
                         int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, ani_signeighbor_t *out, int32_t *count)
{
  return screen_entry(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, false, -1, out, count);
}

int ani_signature_screen_contain(ani_ctx *ctx, const uint32_t *refSig, const int32_t *refLen, int32_t nRef, const uint32_t *qrySig, const int32_t *qryLen,
                                 int32_t nQry, int32_t size, int32_t kmerSize, int32_t minShared, float minIdentity, int32_t k, int32_t mode, ani_signeighbor_t *out,
                                 int32_t *count)
{
  return screen_entry(ctx, refSig, refLen, nRef, qrySig, qryLen, nQry, size, kmerSize, minShared, minIdentity, k, true, mode, out, count);
}

int ani_signature_screen_strips(const ani_ctx *ctx) { return ctx ? ctx->sigScreenStrips : 0; }

void ani_signature_screen_tile(const ani_ctx *ctx, int32_t *tileQueries, int32_t *tileRefs)
{
  if (tileQueries) *tileQueries = ctx ? ctx->sigScreenTile[0] : 0;
  if (tileRefs) *tileRefs = ctx ? ctx->sigScreenTile[1] : 0;
}

// the two cluster calls: the checks of ani_signature_cluster's rules 6 - 8 and, with `contain`, of the mode, then the call; without
// `contain` it is ani_signature_cluster and the mode plays no part
static int cluster_entry(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                         float minIdentity, bool contain, int32_t mode, int32_t *representative, ani_signeighbor_t *link)
{
  if (!ctx) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  TRY(sig_check_sizes(size, kmerSize));
  if (minShared < 1) return fail(ANI_ERR_ARG, "minShared %d below 1", minShared);
  if (!(minIdentity > 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside (0, 100]", (double)minIdentity);
  if (contain && (mode < ANI_CONTAIN_QUERY || mode > ANI_CONTAIN_MAX)) return fail(ANI_ERR_ARG, "containment mode %d outside [0, 2]", mode);
  if (contain && mode != ANI_CONTAIN_MAX)
    return fail(ANI_ERR_ARG, "containment mode %d: the greedy rule needs a symmetric estimate, ANI_CONTAIN_MAX", mode);
  if (nGenomes > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d genomes: the clustering takes at most 2^30", nGenomes);
  for (uint64_t &x : ctx->sigClusterStats) x = 0;
  if (nGenomes == 0) return ANI_OK;
  if (!sig || !len || !representative || !link) return fail(ANI_ERR_ARG, "null argument");
  TRY(sig_check_lengths(len, nGenomes, size, ""));
  HIP_TRY(hipSetDevice(ctx->device));
  try {
    if (contain) return signature_cluster_contain(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, mode, representative, link);
    return signature_cluster(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, representative, link);
  }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_signature_cluster(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                          float minIdentity, int32_t *representative, ani_signeighbor_t *link)
{
  return cluster_entry(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, false, -1, representative, link);
}

int ani_signature_cluster_contain(ani_ctx *ctx, const uint32_t *sig, const int32_t *len, int32_t nGenomes, int32_t size, int32_t kmerSize, int32_t minShared,
                                  float minIdentity, int32_t mode, int32_t *representative, ani_signeighbor_t *link)
{
  return cluster_entry(ctx, sig, len, nGenomes, size, kmerSize, minShared, minIdentity, true, mode, representative, link);
}

int ani_signature_cluster_stats(const ani_ctx *ctx, uint64_t out[4])
{
  if (!out) return fail(ANI_ERR_ARG, "null argument");
  for (int i = 0; i < 4; i++) out[i] = ctx ? ctx->sigClusterStats[i] : 0;
  return ANI_OK;
}

}  // extern "C"
