// profile.hpp — per-bin conservation profile of the reference genomes (ani_sketch_profile_begin / _read; no counterpart in the
// reference, which folds the bin table of computeCoreIdentity.hpp:237-254 into a row and drops it).  DESIGN.md section 2.23.
//
// reduce_stage leaves the bin table of a sub-batch in ctx->bins ([nQuery][bins of the index chunk]: cell = the best bidirectional
// identity of the query in that bin, 0 = empty) and the pair table in ctx->rows ((countSeq, identity bits) per (query, genome)).
// A pair contributes iff it has a row, countSeq >= minFragments and bits(identity) >= bits(minIdentity); per contributing pair
//   queries[g] += 1, and for every non-empty cell of g: count[b] += 1, sum[b] += fix(cell), min[b] / max[b] by bit pattern,
//   fix(x) = llrint((double)x * 2^20) — integer sums: the result depends on no order.
// One lane owns one bin (k_profile_bins) or one genome (k_profile_queries) over every row of the table and does one
// read-modify-write of the chunk's accumulators: a launch has one owner per accumulator and the launches of a context are serial
// on its stream, so there are no atomics.  count and queries saturate at 2^32 - 1 (ani_sketch_profile_read reports that value).
#pragma once
#include "common.hpp"

namespace ani {

constexpr uint32_t kProfileFull = 0xffffffffu;      // a saturated counter; also the `min` of a bin nothing has reached yet

struct ProfileArgs {
  int32_t nQuery, nRefGenomes;
  const uint32_t *bins; size_t binsPerQuery;   // the chunk's bin table, binsPerQuery == the chunk's totalBins
  const uint32_t *genomeBinStart;              // [nRefGenomes + 1]
  const uint32_t *pairCount, *pairIdentity; int32_t outStride, outCol0;      // as PairArgs (reduce.hpp) wrote them
  uint32_t minIdBits, minFragments;            // the gate
  // the chunk's accumulators
  uint32_t *count, *minBits, *maxBits; unsigned long long *sum;    // [totalBins]
  uint32_t *queries;                                               // [nRefGenomes]
};

__device__ __forceinline__ uint32_t profile_add_sat(uint32_t a, uint32_t b)
{
  const unsigned long long s = (unsigned long long)a + b;
  return s >= kProfileFull ? kProfileFull : (uint32_t)s;
}

__device__ __forceinline__ bool profile_gate(const ProfileArgs &a, size_t o)
{
  const uint32_t c = a.pairCount[o];
  return c != 0 && c >= a.minFragments && a.pairIdentity[o] >= a.minIdBits;     // identities are positive floats: bits order like uints
}

// one lane per bin of the chunk; a workgroup reads 256 consecutive cells of every query row (one coalesced 1 KB load per row)
static __global__ __launch_bounds__(kTPB) void k_profile_bins(ProfileArgs a)
{
  const size_t b = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (b >= a.binsPerQuery) return;
  // the genome of the bin: the last g with genomeBinStart[g] <= b
  int lo = 0, hi = a.nRefGenomes;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.genomeBinStart[mid] <= (uint32_t)b) lo = mid; else hi = mid;
  }
  const size_t col = (size_t)(a.outCol0 + lo);
  uint32_t cnt = 0, mn = kProfileFull, mx = 0;
  unsigned long long sum = 0;
  const uint32_t *cell = a.bins + b;
  for (int q = 0; q < a.nQuery; q++, cell += a.binsPerQuery) {
    const uint32_t bits = *cell;
    if (!bits) continue;                                   // nearly every cell
    if (!profile_gate(a, (size_t)q * (size_t)a.outStride + col)) continue;
    cnt++;
    sum += (unsigned long long)llrint((double)__uint_as_float(bits) * 1048576.0);
    mn = bits < mn ? bits : mn; mx = bits > mx ? bits : mx;
  }
  if (!cnt) return;
  a.count[b] = profile_add_sat(a.count[b], cnt);
  a.sum[b] += sum;
  if (mn < a.minBits[b]) a.minBits[b] = mn;
  if (mx > a.maxBits[b]) a.maxBits[b] = mx;
}

// one lane per genome of the chunk: the rows of the pair table that pass the gate (consecutive lanes read consecutive columns)
static __global__ __launch_bounds__(kTPB) void k_profile_queries(ProfileArgs a)
{
  const int g = blockIdx.x * kTPB + threadIdx.x;
  if (g >= a.nRefGenomes) return;
  uint32_t n = 0;
  for (int q = 0; q < a.nQuery; q++) n += profile_gate(a, (size_t)q * (size_t)a.outStride + (size_t)(a.outCol0 + g)) ? 1u : 0u;
  if (n) a.queries[g] = profile_add_sat(a.queries[g], n);
}

}  // namespace ani
