// ci.hpp — percentile bootstrap intervals of the ANI values (ani_sketch_ci_begin / _take; no counterpart in the reference, which prints
// the mean of a pair's cells and nothing about how far to trust it).  DESIGN.md section 2.26.
//
// reduce_stage leaves the bin table of a sub-batch in ctx->bins and the pair table in ctx->rows (see profile.hpp).  For every pair that
// passes the gate (a row, countSeq >= minFragments, bits(identity) >= bits(minIdentity)) the non-empty cells of the genome's bins, in
// bin order, are the sample: F[i] = fix(cell i) = llrint((double)cell * 2^20), an integer below 2^27.  Replicate r draws `count`
// positions with a counter-based hash of (seed, r, j, count) — fmix32, MurmurHash3's finalizer — and adds the F there up to S[r]; the
// record holds the two order statistics of S[0 .. B) the level asks for.  Everything after fix is integer: no result depends on an order.
//   k_ci_flags    one lane per (query, genome of the chunk): the gate -> a flag; device_scan turns flags into offsets;
//   k_ci_list     the gated pairs, in (query, genome) order, into a list, and per listed pair the cells it needs in the device pool
//                 (its countSeq if that is above the LDS cap, else 0); a second device_scan gives the pool offsets;
//   k_ci_records  one workgroup of 256 per listed pair.  It walks the genome's bins 256 at a time; the waves' ballots of the non-empty
//                 lanes, their popcounts through LDS and a prefix popcount give each cell its slot — bin order without a sort — and F
//                 goes to LDS — or, for a pair with more cells than the cap, to the pair's run of the pool — with minimum, maximum and
//                 sum on the way (one wave walking 64 bins at a time left most of the kernel waiting for that one load).  A pair whose
//                 minimum equals its maximum is done (every replicate is the sum).  Else thread t takes the replicates t, t + 256, ...:
//                 one fmix32, one multiply-high and one read of F per draw, the 64-bit sum in registers, S[r] into LDS.  The order
//                 statistics come by counting: thread t counts the u with (S[u], u) < (S[t], t), every read of S[u] a broadcast, and
//                 the thread whose count is the rank stores its sum.  No floating point after fix, no scratch.
// LDS: 2560 cells (10 KiB) + 1024 sums (8 KiB): eight workgroups, the 32 waves a CU takes, in 145 of its 160 KiB.  2560 cells are a
// genome of 7.6 Mbp at the default fragment length all of whose bins a query reaches; the pool path is the same code on global memory.
#pragma once
#include "common.hpp"

namespace ani {

constexpr int kCiMaxReplicates = 1024;
constexpr int kCiLdsCells = 2560;

struct CiArgs {
  int32_t nQuery, nRefGenomes;
  const uint32_t *bins; size_t binsPerQuery;   // the chunk's bin table
  const uint32_t *genomeBinStart;              // [nRefGenomes + 1]
  const uint32_t *pairCount, *pairIdentity; int32_t outStride, outCol0;      // as PairArgs (reduce.hpp) wrote them
  uint32_t minIdBits, minFragments;            // the gate
  int32_t genomeBase;                          // set-global id of the chunk's first genome
  uint32_t replicates, lowRank, highRank, seed;
  uint32_t ldsCells;                           // pairs with more cells than this keep them in the pool (<= kCiLdsCells)
};

// one record as the host receives it (ani_ci_t of ani_abi.h; qry = the query's index in the sub-batch; low and high are the host's)
struct CiRec { int32_t ref, qry; uint32_t count, replicates; unsigned long long sum, lowSum, highSum; float low, high; };
static_assert(sizeof(CiRec) == 48, "record layout");

__device__ __forceinline__ bool ci_gate(const CiArgs &a, size_t o)
{
  const uint32_t c = a.pairCount[o];
  return c != 0 && c >= a.minFragments && a.pairIdentity[o] >= a.minIdBits;     // identities are positive floats: bits order like uints
}

__host__ __device__ __forceinline__ uint32_t ci_fmix32(uint32_t h)
{
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// S[r] of the replicate with key k over f[0 .. count)
__device__ __forceinline__ unsigned long long ci_replicate(const uint32_t *f, uint32_t count, uint32_t k)
{
  unsigned long long s = 0;
  uint32_t m = 0x85ebca6bu;                             // 0x85ebca6b (j + 1), mod 2^32
#pragma unroll 4
  for (uint32_t j = 0; j < count; j++, m += 0x85ebca6bu) s += f[__umulhi(ci_fmix32(k ^ m), count)];
  return s;
}

// The non-empty cells of genome g's bins for query qi, in bin order -> F[0 .. count) in sF, or in gF for a pair above the cap (`big`,
// block-uniform), with the minimum and the maximum of the cells' bits and the sum of the F, the same in every thread on return: a slab
// of 256 bins per turn, the next slab's load in flight over the barrier.  For a workgroup of kTPB threads, all of them (barriers inside);
// the cells are visible to every thread on return.  Shared with kernels/boot.hpp.
__device__ __forceinline__ void ci_gather(const CiArgs &a, int qi, int g, uint32_t count, bool big, uint32_t *gF, uint32_t *sF,
                                          uint32_t (*sCnt)[kTPB / kWave], uint32_t *sMin, uint32_t *sMax, unsigned long long *sSum,
                                          uint32_t &mn, uint32_t &mx, unsigned long long &sum)
{
  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const uint32_t *b = a.bins + (size_t)qi * a.binsPerQuery;
  const uint32_t xg = a.genomeBinStart[g], x1 = a.genomeBinStart[g + 1];
  uint32_t at = 0, turn = 0;
  mn = 0xffffffffu; mx = 0; sum = 0;
  uint32_t next = (xg + t < x1) ? b[xg + t] : 0u;
  for (uint32_t x0 = xg; x0 < x1; x0 += kTPB, turn ^= 1u) {       // block-uniform bounds
    const uint32_t bits = next;
    next = (x1 - x0 > (uint32_t)kTPB + t) ? b[x0 + kTPB + t] : 0u;
    const unsigned long long m = __ballot(bits != 0);
    if (lane == 0) sCnt[turn][wv] = (uint32_t)__popcll(m);
    __syncthreads();                                    // (sCnt[turn] is written again two turns on, behind the next turn's barrier)
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)(kTPB / kWave); w++) { const uint32_t c = sCnt[turn][w]; before += w < wv ? c : 0u; all += c; }
    const uint32_t slot = at + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (bits && slot < count) {                         // (slot < count always: countSeq is the number of these cells)
      const uint32_t f = (uint32_t)llrint((double)__uint_as_float(bits) * 1048576.0);
      if (big) gF[slot] = f; else sF[slot] = f;
      mn = bits < mn ? bits : mn; mx = bits > mx ? bits : mx; sum += f;
    }
    at += all;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d);
    const unsigned long long os = __shfl_xor(sum, d);
    mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; sum += os;
  }
  if (lane == 0) { sMin[wv] = mn; sMax[wv] = mx; sSum[wv] = sum; }
  __syncthreads();                                      // the workgroup's own writes to the pool are visible to it behind the barrier
  sum = 0;
#pragma unroll
  for (int w = 0; w < kTPB / kWave; w++) { mn = sMin[w] < mn ? sMin[w] : mn; mx = sMax[w] > mx ? sMax[w] : mx; sum += sSum[w]; }
}

// pair index p = query * nRefGenomes + genome of the chunk
static __global__ __launch_bounds__(kTPB) void k_ci_flags(CiArgs a, int32_t *__restrict__ flags)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)a.nQuery * (size_t)a.nRefGenomes) return;
  const size_t qi = p / (size_t)a.nRefGenomes, g = p % (size_t)a.nRefGenomes;
  flags[p] = ci_gate(a, qi * (size_t)a.outStride + (size_t)a.outCol0 + g) ? 1 : 0;
}

// the gated pairs, in (query, genome) order, and the pool cells each needs
static __global__ __launch_bounds__(kTPB) void k_ci_list(CiArgs a, const int32_t *__restrict__ flags, const uint32_t *__restrict__ off,
                                                  uint32_t *__restrict__ list, int32_t *__restrict__ poolCells)
{
  const size_t p = (size_t)blockIdx.x * kTPB + threadIdx.x;
  if (p >= (size_t)a.nQuery * (size_t)a.nRefGenomes || !flags[p]) return;
  const size_t qi = p / (size_t)a.nRefGenomes, g = p % (size_t)a.nRefGenomes;
  const uint32_t c = a.pairCount[qi * (size_t)a.outStride + (size_t)a.outCol0 + g];
  list[off[p]] = (uint32_t)p;
  poolCells[off[p]] = c > a.ldsCells ? (int32_t)c : 0;
}

// pairs [first, first + n) of the list -> rec[0 .. n); a pair above the cap keeps its cells at pool[poolOff[pair] - poolBase ..)
static __global__ __launch_bounds__(kTPB) void k_ci_records(CiArgs a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ poolOff,
                                                     uint32_t first, uint32_t n, uint32_t poolBase, uint32_t *pool, CiRec *__restrict__ rec)
{
  __shared__ uint32_t sF[kCiLdsCells];
  __shared__ unsigned long long sS[kCiMaxReplicates];
  __shared__ unsigned long long sSum[kTPB / kWave], sLow, sHigh;
  __shared__ uint32_t sCnt[2][kTPB / kWave], sMin[kTPB / kWave], sMax[kTPB / kWave];
  const uint32_t r = blockIdx.x;
  if (r >= n) return;                                   // block-uniform
  const uint32_t t = threadIdx.x;
  const uint32_t p = list[first + r];
  const int qi = (int)(p / (uint32_t)a.nRefGenomes), g = (int)(p % (uint32_t)a.nRefGenomes);
  const uint32_t count = a.pairCount[(size_t)qi * (size_t)a.outStride + (size_t)a.outCol0 + (size_t)g];   // = the non-empty cells of g
  const bool big = count > a.ldsCells;                  // block-uniform
  uint32_t *gF = pool + (big ? poolOff[first + r] - poolBase : 0u);

  uint32_t mn, mx;
  unsigned long long sum;
  ci_gather(a, qi, g, count, big, gF, sF, sCnt, sMin, sMax, sSum, mn, mx, sum);

  const uint32_t B = a.replicates;
  unsigned long long lowSum = sum, highSum = sum;
  if (mn != mx) {                                       // block-uniform; one distinct value: every replicate is the sum
    for (uint32_t q = t; q < B; q += kTPB) {
      const uint32_t k = ci_fmix32(a.seed + 0x9e3779b9u * (q + 1u));
      sS[q] = big ? ci_replicate(gF, count, k) : ci_replicate(sF, count, k);
    }
    __syncthreads();
    for (uint32_t q = t; q < B; q += kTPB) {
      const unsigned long long s = sS[q];
      uint32_t rank = 0;
      for (uint32_t u = 0; u < B; u++) { const unsigned long long o = sS[u]; rank += (o < s || (o == s && u < q)) ? 1u : 0u; }
      if (rank == a.lowRank) sLow = s;                  // the ranks under (S, replicate) are a permutation: one writer each
      if (rank == a.highRank) sHigh = s;
    }
    __syncthreads();
    lowSum = sLow; highSum = sHigh;
  }
  if (t == 0) {
    CiRec o;
    o.ref = a.genomeBase + g; o.qry = qi; o.count = count; o.replicates = B; o.sum = sum; o.lowSum = lowSum; o.highSum = highSum; o.low = 0.0f; o.high = 0.0f;
    rec[r] = o;
  }
}

}  // namespace ani
