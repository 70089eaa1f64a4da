// fragdist.hpp — per-pair fragment identity distributions (ani_sketch_fragdist_begin / _take; no counterpart in the reference, which
// folds the bin table of computeCoreIdentity.hpp:237-254 into a mean per pair and drops it).  DESIGN.md section 2.24.
//
// reduce_stage leaves the bin table of a sub-batch in ctx->bins and the pair table in ctx->rows (see profile.hpp).  For every pair
// that passes the gate (a row, countSeq >= minFragments, bits(identity) >= bits(minIdentity)) one record is made from the non-empty
// cells of the genome's bins: their count, a histogram over caller-given class edges, minimum, quartiles, median and maximum by bit
// pattern and the sum of fix(cell) = llrint((double)cell * 2^20).  Everything is integer or bit pattern: no result depends on an order.
//
// Nearly every pair of a large run has no row, so the shape is compact, then work:
//   k_fragdist_flags   one lane per (query, genome of the chunk): the gate -> a flag; device_scan turns flags into offsets;
//   k_fragdist_list    the gated pairs, in (query, genome) order, into a list;
//   k_fragdist_records one wave (= one workgroup of 64: its barriers are the wave's own) per listed pair.  Four walks over the genome's
//                      bins, 64 at a time as k_pair_reduce reads them.  The first classifies every cell by binary search over the edges
//                      (in LDS) into a per-wave LDS histogram, keeps per-lane minimum, maximum and sum, and counts the top byte of the
//                      bit patterns; the other three finish a radix select of 8 bits per round for the three inner ranks together
//                      (3 x 256 LDS counters: a cell counts for rank k iff its upper bits equal k's prefix so far); a pair whose
//                      minimum equals its maximum skips them.  One path for every bin count; no scratch.
#pragma once
#include "common.hpp"

namespace ani {

constexpr int kFragDistMaxEdges = 63;                // at most 64 classes: lane c writes class c

struct FragDistArgs {
  int32_t nQuery, nRefGenomes;
  const uint32_t *bins; size_t binsPerQuery;   // the chunk's bin table
  const uint32_t *genomeBinStart;              // [nRefGenomes + 1]
  const uint32_t *pairCount, *pairIdentity; int32_t outStride, outCol0;      // as PairArgs (reduce.hpp) wrote them
  uint32_t minIdBits, minFragments;            // the gate
  int32_t genomeBase;                          // set-global id of the chunk's first genome
  int32_t nEdges;
  uint32_t edgeBits[kFragDistMaxEdges];        // the bit patterns of the edges, ascending
};

// one record as the host receives it (ani_fragdist_t of ani_abi.h, identities as bits; qry = the query's index in the sub-batch)
struct FragDistRec { int32_t ref, qry; uint32_t count, mn, q1, med, q3, mx; unsigned long long sum; };
static_assert(sizeof(FragDistRec) == 40, "record layout");

__device__ __forceinline__ bool fragdist_gate(const FragDistArgs &a, size_t o)
{
  const uint32_t c = a.pairCount[o];
  return c != 0 && c >= a.minFragments && a.pairIdentity[o] >= a.minIdBits;     // identities are positive floats: bits order like uints
}

// pair index p = query * nRefGenomes + genome of the chunk
static __global__ __launch_bounds__(kTPB) void k_fragdist_flags(FragDistArgs a, int32_t *__restrict__ flags)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)a.nQuery * (size_t)a.nRefGenomes) return;
  const size_t qi = p / (size_t)a.nRefGenomes, g = p % (size_t)a.nRefGenomes;
  flags[p] = fragdist_gate(a, qi * (size_t)a.outStride + (size_t)a.outCol0 + g) ? 1 : 0;
}

static __global__ __launch_bounds__(kTPB) void k_fragdist_list(uint32_t nPairs, const int32_t *__restrict__ flags, const uint32_t *__restrict__ off,
                                                        uint32_t *__restrict__ list)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p < nPairs && flags[p]) list[off[p]] = (uint32_t)p;
}

// records [first, first + n) of the list -> rec[0 .. n), hist[0 .. n)[nEdges + 1]
static __global__ __launch_bounds__(kWave) void k_fragdist_records(FragDistArgs a, const uint32_t *__restrict__ list, uint32_t first, uint32_t n,
                                                            FragDistRec *__restrict__ rec, uint32_t *__restrict__ hist)
{
  __shared__ uint32_t sEdge[kWave], sHist[kWave], sCnt[3 * 256], sSel[6];
  const uint32_t r = blockIdx.x;
  if (r >= n) return;                                   // block-uniform
  const int lane = threadIdx.x;
  const uint32_t p = list[first + r];
  const int qi = (int)(p / (uint32_t)a.nRefGenomes), g = (int)(p % (uint32_t)a.nRefGenomes);
  const uint32_t *b = a.bins + (size_t)qi * a.binsPerQuery;
  const uint32_t x0g = a.genomeBinStart[g], x1 = a.genomeBinStart[g + 1];
  const int nE = a.nEdges;
  sEdge[lane] = lane < nE ? a.edgeBits[lane] : 0xffffffffu;
  sHist[lane] = 0;
  for (int i = lane; i < 256; i += kWave) sCnt[i] = 0;
  __syncthreads();

  // first walk: classes, minimum, maximum, sum, count, and the top byte of the select
  uint32_t mn = 0xffffffffu, mx = 0, cnt = 0;
  unsigned long long sum = 0;
  for (uint32_t x0 = x0g; x0 < x1; x0 += kWave) {
    const uint32_t bits = (x0 + lane < x1) ? b[x0 + lane] : 0u;
    cnt += (uint32_t)__popcll(__ballot(bits != 0));
    if (bits) {
      int lo = 0, hi = nE;                              // class = the number of edges <= bits: the first edge above it
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (sEdge[mid] <= bits) lo = mid + 1; else hi = mid; }
      atomicAdd(&sHist[lo], 1u);
      atomicAdd(&sCnt[bits >> 24], 1u);
      mn = bits < mn ? bits : mn; mx = bits > mx ? bits : mx;
      sum += (unsigned long long)llrint((double)__uint_as_float(bits) * 1048576.0);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d);
    const unsigned long long os = __shfl_xor(sum, d);
    mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; sum += os;
  }
  __syncthreads();

  // radix select of ranks (c-1)/4, (c-1)/2, 3(c-1)/4 (cnt >= 1: the pair has a row), 8 bits a round; all of it wave-uniform
  // (one distinct value - the single cell of nearly every row between unrelated genomes - is every rank's answer: no further walk)
  uint32_t rank[3] = {(cnt - 1) / 4, (cnt - 1) / 2, (uint32_t)(3ull * (cnt - 1) / 4)}, prefix[3] = {0, 0, 0};
  if (mn == mx) prefix[0] = prefix[1] = prefix[2] = mn;
  else for (int round = 0; round < 4; round++) {
    if (round) {
      const int shift = 24 - 8 * round;
      for (uint32_t x0 = x0g; x0 < x1; x0 += kWave) {
        const uint32_t bits = (x0 + lane < x1) ? b[x0 + lane] : 0u;
        if (!bits) continue;
        const uint32_t up = bits >> (shift + 8), dg = (bits >> shift) & 255u;
#pragma unroll
        for (int k = 0; k < 3; k++) if (up == prefix[k]) atomicAdd(&sCnt[k * 256 + dg], 1u);
      }
      __syncthreads();
    }
    // per rank: the digit whose run of the counters holds the rank; lane l owns counters 4l .. 4l + 3
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t *t = sCnt + (round ? k * 256 : 0);
      const uint32_t c0 = t[4 * lane], c1 = t[4 * lane + 1], c2 = t[4 * lane + 2], c3 = t[4 * lane + 3];
      const uint32_t tot = c0 + c1 + c2 + c3;
      uint32_t incl = tot;
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) { const uint32_t o = __shfl_up(incl, d); if (lane >= d) incl += o; }
      const uint32_t excl = incl - tot;
      if (excl <= rank[k] && rank[k] < incl) {          // one lane: the ranks lie below the number of cells the counters hold
        uint32_t rr = rank[k] - excl; int j = 0;
        if (rr >= c0) { rr -= c0; j = 1; if (rr >= c1) { rr -= c1; j = 2; if (rr >= c2) { rr -= c2; j = 3; } } }
        sSel[2 * k] = (uint32_t)(4 * lane + j); sSel[2 * k + 1] = rr;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) { prefix[k] = (prefix[k] << 8) | sSel[2 * k]; rank[k] = sSel[2 * k + 1]; }
    __syncthreads();
    if (round < 3) {
      for (int i = lane; i < 3 * 256; i += kWave) sCnt[i] = 0;
      __syncthreads();
    }
  }

  if (lane == 0) {
    FragDistRec o;
    o.ref = a.genomeBase + g; o.qry = qi; o.count = cnt; o.mn = mn; o.q1 = prefix[0]; o.med = prefix[1]; o.q3 = prefix[2]; o.mx = mx; o.sum = sum;
    rec[r] = o;
  }
  if (lane <= nE) hist[(size_t)r * (size_t)(nE + 1) + lane] = sHist[lane];
}

}  // namespace ani
