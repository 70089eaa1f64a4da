// synteny.hpp — collinear blocks and breakpoints of a pair's reciprocal best hits (ani_sketch_synteny_begin / _take; the reference shows
// the order of the hits only as the dot plot of --visualize, one pair per run).  DESIGN.md section 2.28.
//
// reduce_stage leaves the bin table of a sub-batch in ctx->bins and the pair table in ctx->rows; the owner and claim passes of hits.hpp,
// run under THIS mode's gate, leave the winning candidate of every non-empty cell of every gated pair in the owner table.  A pair's hits
// are those cells in bin order; everything below is integer arithmetic on (querySeqId, contig, refStartPos, fix(identity)) of the hits.
//   k_syn_list     the gated pairs in (query, genome) order with their countSeq (= hits = an upper bound of their blocks) and, for a pair
//                  above the LDS cap, the 8-byte units it needs in the device pool; device_scan gives record and pool offsets;
//   k_syn_pairs    one workgroup of 256 per listed pair.
//                  1. the non-empty cells go to the work arrays in bin order by ballot and prefix popcount (as k_ci_records gathers
//                     cells): the owner's candidate, and the sort key querySeqId << 32 | position;
//                  2. a bitonic sort of the keys, padded with ~0 to a power of two; the sorted position scattered back is the hit's rank
//                     among the pair's own querySeqIds;
//                  3. P[i], the inclusive prefix sum of fix(identity) in bin order, takes the place of the keys;
//                  4. one pass over the adjacencies: each is classified, block starts are marked; per slab of 256 hits the waves'
//                     ballots give every hit the number of starts up to it (its block index) and the position of the last start up to
//                     it (a max-scan of start positions, read off the ballot mask); the LAST hit of a block writes the block record,
//                     idSum = P[last] - P[first - 1];
//                  5. workgroup reductions fill the pair record.
//                  The block records go to a pool at the pair's HIT offset (blocks <= hits); the pair's block count goes to a list;
//   k_syn_compact  after a device_scan over the piece's block counts: one workgroup per pair moves its blocks to their final place.
// One launch plus a compaction, not a counting launch and a writing launch: the gather and the sort, which are the cost, run once, and the
// compaction moves 32 bytes per block.
// LDS: 2048 keys / prefix sums (16 KiB), candidates (8 KiB), ranks (8 KiB) and 256 bytes of scan scratch: four workgroups, 16 waves, in
// 129 of the 160 KiB of a CU.  A pair with more hits than the cap runs the same code on its run of the device pool.  No scratch.
#pragma once
#include "common.hpp"
#include "hits.hpp"

namespace ani {

constexpr int kSynLdsHits = 2048;
constexpr int kSynWaves = kTPB / kWave;

struct SynArgs {
  HitsArgs h;                                  // candidates, bin table, pair table, owner table — and this mode's gate
  uint32_t ldsHits;                            // pairs with more hits than this work in the pool (<= kSynLdsHits)
};

// the records as the host receives them (ani_synteny_t and ani_synblock_t of ani_abi.h; qry = the query's index in the sub-batch)
struct SynRec { int32_t ref, qry; uint32_t count, forward, reverse, breaks, contigBorders, blocks, reverseBlocks, reverseHits, largestBlock, singletons; };
struct SynBlock { int32_t refSeq, refStartFirst, refStartLast, qSeqFirst, qSeqLast; uint32_t hits; unsigned long long idSum; };
static_assert(sizeof(SynRec) == 48 && sizeof(SynBlock) == 32, "record layout");

constexpr uint32_t kSynNoCand = 0xffffffffu;

__host__ __device__ __forceinline__ uint32_t syn_pad(uint32_t n)              // the sort's length: the power of two at or above n (n <= 2^31)
{
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
// 8-byte units of a pooled pair: keys [pad], then candidates and ranks [n each, rounded up to whole units]
__host__ __device__ __forceinline__ uint32_t syn_pool_units(uint32_t n) { return syn_pad(n) + 2u * ((n + 1u) / 2u); }

// adjacency classes, in the ABI's order
enum { kSynForward = 0, kSynReverse = 1, kSynBreak = 2, kSynContig = 3 };
__device__ __forceinline__ int syn_class(int32_t c0, int32_t c1, uint32_t r0, uint32_t r1)
{
  if (c0 != c1) return kSynContig;
  if (r1 == r0 + 1u) return kSynForward;
  if (r1 + 1u == r0) return kSynReverse;
  return kSynBreak;
}

__device__ __forceinline__ int32_t syn_contig(const HitsArgs &h, uint32_t c) { return c != kSynNoCand ? h.w.candSeq[c] : -1; }
__device__ __forceinline__ uint32_t syn_fix(const HitsArgs &h, uint32_t c)
{
  return c != kSynNoCand ? (uint32_t)llrint((double)__uint_as_float(h.w.idBits[c]) * 1048576.0) : 0u;
}

// the gated pairs, in (query, genome) order: countSeq and the pool units each needs
static __global__ __launch_bounds__(kTPB) void k_syn_list(SynArgs a, const int32_t *__restrict__ flags, const uint32_t *__restrict__ off,
                                                   uint32_t *__restrict__ list, int32_t *__restrict__ count, int32_t *__restrict__ poolUnits)
{
  const HitsArgs &h = a.h;
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)h.nQuery * (size_t)h.nRefGenomes || !flags[p]) return;
  const size_t qi = p / (size_t)h.nRefGenomes, g = p % (size_t)h.nRefGenomes;
  const uint32_t c = h.pairCount[qi * (size_t)h.outStride + (size_t)h.outCol0 + g];
  list[off[p]] = (uint32_t)p;
  count[off[p]] = (int32_t)c;
  poolUnits[off[p]] = c > a.ldsHits ? (int32_t)syn_pool_units(c) : 0;
}

// one pair on its work arrays (LDS or the pair's run of the pool; inlined once for each, so that every access knows its address space)
__device__ __forceinline__ void syn_pair(const SynArgs &a, int qi, int g, uint32_t count, unsigned long long *key, uint32_t *cand, uint32_t *rank,
                                         uint32_t (*sW)[kSynWaves][2], unsigned long long (*sTot)[kSynWaves], uint32_t (*sRed)[kSynWaves],
                                         SynRec *rec, SynBlock *blk, int32_t *blkCount)
{
  const HitsArgs &h = a.h;
  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;

  // 1. the cells in bin order -> cand[0 .. count), key[0 .. count)
  const uint32_t *b = h.w.bins + (size_t)qi * h.w.binsPerQuery;
  const uint32_t *ow = h.owner + (size_t)qi * h.w.binsPerQuery;
  const uint32_t xg = h.genomeBinStart[g], x1 = h.genomeBinStart[g + 1];
  uint32_t at = 0, turn = 0;
  for (uint32_t x0 = xg; x0 < x1; x0 += kTPB, turn ^= 1u) {         // block-uniform bounds
    const uint32_t bits = (t < x1 - x0) ? b[x0 + t] : 0u;
    const unsigned long long m = __ballot(bits != 0);
    if (lane == 0) sW[turn][wv][0] = (uint32_t)__popcll(m);
    __syncthreads();                                    // (sW[turn] is written again two turns on, behind the next turn's barrier)
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kSynWaves; w++) { const uint32_t c = sW[turn][w][0]; before += w < wv ? c : 0u; all += c; }
    const uint32_t slot = at + before + (uint32_t)__popcll(m & below);
    if (bits && slot < count) {                         // (slot < count always: countSeq is the number of these cells)
      const uint32_t o = ow[x0 + t];
      const uint32_t c = ((o & kHitClaimed) && (o & ~kHitClaimed) < (uint32_t)h.w.nCand) ? (o & ~kHitClaimed) : kSynNoCand;   // (claimed always)
      const uint32_t q = c != kSynNoCand ? (uint32_t)h.fragQSeq[h.w.candFrag[c]] : 0xffffffffu;
      cand[slot] = c;
      key[slot] = ((unsigned long long)q << 32) | slot;
    }
    at += all;
    if (x1 - x0 <= (uint32_t)kTPB) break;               // (x0 += kTPB must not wrap)
  }
  const uint32_t n2 = syn_pad(count);
  for (uint32_t i = count + t; i < n2; i += kTPB) key[i] = ~0ull;
  __syncthreads();

  // 2. bitonic sort of key[0 .. n2): n2 / 2 comparators per step; the padding is above every key (querySeqId < 2^31) and stays behind
  for (unsigned long long k = 2; k <= n2; k <<= 1)
    for (uint32_t j = (uint32_t)(k >> 1); j > 0; j >>= 1) {
      for (uint32_t c = t; c < n2 / 2u; c += kTPB) {
        const uint32_t i = ((c & ~(j - 1u)) << 1) | (c & (j - 1u)), l = i | j;
        const unsigned long long u = key[i], v = key[l];
        if ((u > v) == ((i & (uint32_t)k) == 0u)) { key[i] = v; key[l] = u; }
      }
      __syncthreads();
    }
  // the sorted position, scattered back: rank among the pair's own querySeqIds
  for (uint32_t s = t; s < count; s += kTPB) rank[(uint32_t)key[s]] = s;
  __syncthreads();

  // 3. key[i] <- P[i] = fix(0) + ... + fix(i)
  unsigned long long run = 0;
  turn = 0;
  for (uint32_t x0 = 0; x0 < count; x0 += kTPB, turn ^= 1u) {
    const uint32_t i = x0 + t;
    unsigned long long v = (t < count - x0) ? syn_fix(h, cand[i]) : 0u;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) { const unsigned long long o = __shfl_up(v, d); if ((int)lane >= d) v += o; }
    if (lane == kWave - 1) sTot[turn][wv] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kSynWaves; w++) { const unsigned long long c = sTot[turn][w]; before += w < wv ? c : 0ull; all += c; }
    if (t < count - x0) key[i] = run + before + v;
    run += all;
    if (count - x0 <= (uint32_t)kTPB) break;
  }
  __syncthreads();

  // 4. the adjacencies: (i - 1, i) gives hit i its start flag, (i, i + 1) tells whether it ends its block
  uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // forward, reverse, breaks, contig borders; reverse blocks, reverse hits, singletons, largest
  uint32_t blocks = 0, lastStart = 0;
  turn = 0;
  for (uint32_t x0 = 0; x0 < count; x0 += kTPB, turn ^= 1u) {
    const uint32_t i = x0 + t;
    const bool live = t < count - x0;
    bool st = false, last = false;
    uint32_t ri = 0;
    if (live) {
      const int32_t ci = syn_contig(h, cand[i]);
      ri = rank[i];
      if (i == 0) st = true;
      else { const int cl = syn_class(syn_contig(h, cand[i - 1]), ci, rank[i - 1], ri); acc[0] += cl == kSynForward; acc[1] += cl == kSynReverse; acc[2] += cl == kSynBreak; acc[3] += cl == kSynContig;
        st = cl >= kSynBreak; }
      last = i == count - 1 || syn_class(ci, syn_contig(h, cand[i + 1]), ri, rank[i + 1]) >= kSynBreak;
    }
    const unsigned long long m = __ballot(st);
    if (lane == 0) { sW[turn][wv][0] = (uint32_t)__popcll(m); sW[turn][wv][1] = m ? x0 + wv * kWave + 63u - (uint32_t)__clzll(m) : 0xffffffffu; }
    __syncthreads();
    uint32_t before = 0, all = 0, startBefore = lastStart, startAll = lastStart;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kSynWaves; w++) {
      const uint32_t c = sW[turn][w][0], p = sW[turn][w][1];
      before += w < wv ? c : 0u; all += c;
      if (p != 0xffffffffu) { startAll = p; if (w < wv) startBefore = p; }
    }
    if (live && last) {
      const unsigned long long mm = m & (below | (1ull << lane));        // the starts of this wave up to the hit itself
      const uint32_t s = mm ? x0 + wv * kWave + 63u - (uint32_t)__clzll(mm) : startBefore;     // the block's first hit (hit 0 is a start)
      const uint32_t bi = blocks + before + (uint32_t)__popcll(mm) - 1u, n = i - s + 1u;
      const uint32_t c0 = cand[s], c1 = cand[i];
      SynBlock o;
      o.refSeq = c0 != kSynNoCand ? h.seqBase + h.w.candSeq[c0] : -1;
      o.refStartFirst = c0 != kSynNoCand ? h.w.refStart[c0] : -1; o.refStartLast = c1 != kSynNoCand ? h.w.refStart[c1] : -1;
      o.qSeqFirst = c0 != kSynNoCand ? h.fragQSeq[h.w.candFrag[c0]] : -1; o.qSeqLast = c1 != kSynNoCand ? h.fragQSeq[h.w.candFrag[c1]] : -1;
      o.hits = n; o.idSum = key[i] - (s ? key[s - 1] : 0ull);
      if (bi < count) blk[bi] = o;                      // (always: a block has at least one hit)
      if (n == 1u) acc[6]++;
      else if (ri < rank[s]) { acc[4]++; acc[5] += n; }
      acc[7] = n > acc[7] ? n : acc[7];
    }
    blocks += all; lastStart = startAll;
    if (count - x0 <= (uint32_t)kTPB) break;
  }

  // 5. the pair record
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t v = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = k == 7 ? (o > v ? o : v) : v + o; }
    if (lane == 0) sRed[k][wv] = v;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      v[k] = sRed[k][0];
#pragma unroll
      for (int w = 1; w < kSynWaves; w++) v[k] = k == 7 ? (sRed[k][w] > v[k] ? sRed[k][w] : v[k]) : v[k] + sRed[k][w];
    }
    SynRec o;
    o.ref = h.genomeBase + g; o.qry = qi; o.count = count; o.forward = v[0]; o.reverse = v[1]; o.breaks = v[2]; o.contigBorders = v[3];
    o.blocks = blocks; o.reverseBlocks = v[4]; o.reverseHits = v[5]; o.largestBlock = v[7]; o.singletons = v[6];
    *rec = o;
    *blkCount = (int32_t)blocks;
  }
}

// pairs [first, first + n) of the list -> rec[0 .. n), blkCount[0 .. n) and the pair's blocks at blkPool[recOff[pair] - recBase ..); a
// pair above the cap works at pool[poolOff[pair] - poolBase ..) (8-byte units)
static __global__ __launch_bounds__(kTPB) void k_syn_pairs(SynArgs a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ recOff,
                                                    const uint32_t *__restrict__ poolOff, uint32_t first, uint32_t n, uint32_t recBase, uint32_t poolBase,
                                                    unsigned long long *pool, SynRec *__restrict__ rec, SynBlock *__restrict__ blkPool,
                                                    int32_t *__restrict__ blkCount)
{
  __shared__ unsigned long long sKey[kSynLdsHits];
  __shared__ uint32_t sCand[kSynLdsHits], sRank[kSynLdsHits];
  __shared__ unsigned long long sTot[2][kSynWaves];
  __shared__ uint32_t sW[2][kSynWaves][2], sRed[8][kSynWaves];
  const uint32_t r = blockIdx.x;
  if (r >= n) return;                                   // block-uniform
  const HitsArgs &h = a.h;
  const uint32_t p = list[first + r];
  const int qi = (int)(p / (uint32_t)h.nRefGenomes), g = (int)(p % (uint32_t)h.nRefGenomes);
  const uint32_t count = h.pairCount[(size_t)qi * (size_t)h.outStride + (size_t)h.outCol0 + (size_t)g];   // = the non-empty cells of g
  SynBlock *blk = blkPool + (recOff[first + r] - recBase);
  if (count > a.ldsHits) {                              // block-uniform
    unsigned long long *gKey = pool + (poolOff[first + r] - poolBase);
    uint32_t *gCand = (uint32_t *)(gKey + syn_pad(count)), *gRank = gCand + 2u * ((count + 1u) / 2u);
    syn_pair(a, qi, g, count, gKey, gCand, gRank, sW, sTot, sRed, rec + r, blk, blkCount + r);
  } else
    syn_pair(a, qi, g, count, sKey, sCand, sRank, sW, sTot, sRed, rec + r, blk, blkCount + r);
}

// the blocks of pairs [first, first + n) from the pool to out[blkOff[pair] ..), in the pool's order
static __global__ __launch_bounds__(kTPB) void k_syn_compact(const uint32_t *__restrict__ recOff, uint32_t first, uint32_t n, uint32_t recBase,
                                                      const int32_t *__restrict__ blkCount, const uint32_t *__restrict__ blkOff,
                                                      const SynBlock *__restrict__ blkPool, SynBlock *__restrict__ out)
{
  const uint32_t r = blockIdx.x;
  if (r >= n) return;
  const SynBlock *src = blkPool + (recOff[first + r] - recBase);
  SynBlock *dst = out + blkOff[r];
  for (uint32_t k = threadIdx.x; k < (uint32_t)blkCount[r]; k += kTPB) dst[k] = src[k];
}

}  // namespace ani
