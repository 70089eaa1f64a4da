// hits.hpp — reciprocal best-hit records of the fused path (ani_sketch_hits_begin / _take; the reference prints such records for
// --visualize only, from a std::sort on the host: computeCoreIdentity.hpp:214-254).  DESIGN.md section 2.25.
//
// reduce_stage leaves the bin table of a sub-batch in ctx->bins and the pair table in ctx->rows (see profile.hpp); the candidates
// k_oneway_bins folded into the bin table are still in the context's buffers.  For every pair that passes the gate (a row, countSeq >=
// minFragments, bits(identity) >= bits(minIdentity)) one record per non-empty cell is made: the fragment that won the cell — among the
// fragments whose 1-way winner lies in the cell with the cell's identity bits, the one with the largest querySeqId — with the contig,
// start position and identity of that winner.  Everything is integer or bit pattern; nothing depends on an order.
//   k_hits_owner    one lane per candidate; a (fragment, genome) group head resolves its group exactly as k_oneway_bins does and, where
//                   the pair is gated and the group's winner holds the cell's bits, does atomicMax(owner[cell], querySeqId + 1): an
//                   integer maximum, order-free.  `owner` is a second table of the bin table's shape, zeroed per reduce_stage.
//   k_hits_claim    a launch of its own, the same walk: the head whose querySeqId + 1 is the cell's owner stores 0x80000000 | the index
//                   of its winning candidate there.  One writer per cell (querySeqId is unique per fragment of a genome); a head that
//                   lost the cell holds a querySeqId + 1 below the winner's, so below 2^31: the flag bit keeps a stored index from ever
//                   comparing equal to it.  Losers only read.
//   k_hits_flags, k_hits_list   the gated pairs and their countSeq, compacted in (query, genome) order (device_scan between the two); a
//                   second device_scan over the listed counts gives every pair its record offset.
//   k_hits_records  one wave (= one workgroup of 64) per listed pair walks the genome's bins 64 at a time as k_pair_reduce does; the
//                   ballot of the non-empty lanes and a prefix popcount give each cell its slot — (contig, bin) order without a sort —
//                   and the lane fetches the owner's candidate and writes the record.  No LDS, no scratch.
#pragma once
#include "common.hpp"
#include "reduce.hpp"

namespace ani {

struct HitsArgs {
  OneWayArgs w;                                // the candidates and the bin table, as k_oneway_bins got them
  const int32_t *fragQSeq;                     // fragment -> querySeqId
  int32_t nQuery, nRefGenomes;
  const uint32_t *genomeBinStart;              // [nRefGenomes + 1]
  const uint32_t *pairCount, *pairIdentity; int32_t outStride, outCol0;      // as PairArgs (reduce.hpp) wrote them
  uint32_t minIdBits, minFragments;            // the gate
  int32_t genomeBase, seqBase;                 // set-global ids of the chunk's first genome and contig
  uint32_t *owner;                             // [nQuery][binsPerQuery]
};

// one record as the host receives it (ani_hit_t of ani_abi.h, the identity as bits; qry = the query's index in the sub-batch)
struct HitRec { int32_t ref, qry, refSeq, refStart, qSeq; uint32_t idBits; };
static_assert(sizeof(HitRec) == 24, "record layout");

constexpr uint32_t kHitClaimed = 0x80000000u;

__device__ __forceinline__ bool hits_gate(const HitsArgs &a, size_t o)
{
  const uint32_t c = a.pairCount[o];
  return c != 0 && c >= a.minFragments && a.pairIdentity[o] >= a.minIdBits;     // identities are positive floats: bits order like uints
}

// candidate c as a group head: the group's 1-way winner (k_oneway_bins' walk and order), if the pair is gated and the winner holds
// its cell's bits -> the cell, the winning candidate and the fragment's querySeqId + 1; false: no head, no mapping, not gated, or the
// winner lost its cell
__device__ __forceinline__ bool hits_head(const HitsArgs &h, int c, size_t *cell, int *win, uint32_t *key)
{
  const OneWayArgs &a = h.w;
  const int f = a.candFrag[c];
  const int g = a.contigGenome[a.candSeq[c]];
  if (c > 0 && a.candFrag[c - 1] == f && a.contigGenome[a.candSeq[c - 1]] == g) return false;
  uint32_t bBits = 0; int32_t bSeq = -1, bPos = -1; int bAt = -1;
  for (int x = c; x < a.nCand && a.candFrag[x] == f && a.contigGenome[a.candSeq[x]] == g; x++) {
    const uint32_t bits = a.idBits[x];
    if (!bits) continue;
    const int32_t sq = a.candSeq[x], ps = a.refStart[x];
    if (bits > bBits || (bits == bBits && (sq > bSeq || (sq == bSeq && ps > bPos)))) { bBits = bits; bSeq = sq; bPos = ps; bAt = x; }
  }
  if (!bBits) return false;
  const int qi = a.fragGenome[f] - a.genomeBase;
  if (!hits_gate(h, (size_t)qi * (size_t)h.outStride + (size_t)(h.outCol0 + g))) return false;
  const size_t bin = (size_t)qi * a.binsPerQuery + a.contigBinBase[bSeq] + (uint32_t)(bPos / a.binWidth);
  if (a.bins[bin] != bBits) return false;
  *cell = bin; *win = bAt; *key = (uint32_t)h.fragQSeq[f] + 1u;
  return true;
}

static __global__ __launch_bounds__(kTPB) void k_hits_owner(HitsArgs h)
{
  const int c = blockIdx.x * kTPB + threadIdx.x;
  if (c >= h.w.nCand) return;
  size_t cell; int win; uint32_t key;
  if (hits_head(h, c, &cell, &win, &key)) atomicMax(&h.owner[cell], key);
}

static __global__ __launch_bounds__(kTPB) void k_hits_claim(HitsArgs h)
{
  const int c = blockIdx.x * kTPB + threadIdx.x;
  if (c >= h.w.nCand) return;
  size_t cell; int win; uint32_t key;
  if (hits_head(h, c, &cell, &win, &key) && h.owner[cell] == key) h.owner[cell] = kHitClaimed | (uint32_t)win;
}

// pair index p = query * nRefGenomes + genome of the chunk
static __global__ __launch_bounds__(kTPB) void k_hits_flags(HitsArgs h, int32_t *__restrict__ flags)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)h.nQuery * (size_t)h.nRefGenomes) return;
  const size_t qi = p / (size_t)h.nRefGenomes, g = p % (size_t)h.nRefGenomes;
  flags[p] = hits_gate(h, qi * (size_t)h.outStride + (size_t)h.outCol0 + g) ? 1 : 0;
}

// the gated pairs, in (query, genome) order, and their countSeq = their number of records
static __global__ __launch_bounds__(kTPB) void k_hits_list(HitsArgs h, const int32_t *__restrict__ flags, const uint32_t *__restrict__ off,
                                                    uint32_t *__restrict__ list, int32_t *__restrict__ count)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)h.nQuery * (size_t)h.nRefGenomes || !flags[p]) return;
  const size_t qi = p / (size_t)h.nRefGenomes, g = p % (size_t)h.nRefGenomes;
  list[off[p]] = (uint32_t)p;
  count[off[p]] = (int32_t)h.pairCount[qi * (size_t)h.outStride + (size_t)h.outCol0 + g];
}

// pairs [first, first + n) of the list -> their records at out[recOff[pair] - recBase ..), in bin order
static __global__ __launch_bounds__(kWave) void k_hits_records(HitsArgs h, const uint32_t *__restrict__ list, const uint32_t *__restrict__ recOff,
                                                        uint32_t first, uint32_t n, uint32_t recBase, HitRec *__restrict__ out)
{
  const uint32_t r = blockIdx.x;
  if (r >= n) return;                                   // block-uniform
  const int lane = threadIdx.x;
  const uint32_t p = list[first + r];
  const int qi = (int)(p / (uint32_t)h.nRefGenomes), g = (int)(p % (uint32_t)h.nRefGenomes);
  const uint32_t *b = h.w.bins + (size_t)qi * h.w.binsPerQuery;
  const uint32_t *ow = h.owner + (size_t)qi * h.w.binsPerQuery;
  const uint32_t x1 = h.genomeBinStart[g + 1];
  uint32_t at = recOff[first + r] - recBase;
  for (uint32_t x0 = h.genomeBinStart[g]; x0 < x1; x0 += kWave) {
    const uint32_t bits = (x0 + lane < x1) ? b[x0 + lane] : 0u;
    const unsigned long long m = __ballot(bits != 0);
    if (bits) {
      const uint32_t o = ow[x0 + lane], c = o & ~kHitClaimed;
      HitRec rec;
      rec.ref = h.genomeBase + g; rec.qry = qi;
      if ((o & kHitClaimed) && c < (uint32_t)h.w.nCand) {      // every non-empty cell of a gated pair has been claimed
        rec.refSeq = h.seqBase + h.w.candSeq[c]; rec.refStart = h.w.refStart[c]; rec.qSeq = h.fragQSeq[h.w.candFrag[c]]; rec.idBits = h.w.idBits[c];
      } else { rec.refSeq = -1; rec.refStart = -1; rec.qSeq = -1; rec.idBits = 0; }
      out[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = rec;
    }
    at += (uint32_t)__popcll(m);
  }
}

}  // namespace ani
