// tree.hpp — average-linkage (UPGMA) tree of the genomes (ani_tree_average; no counterpart in the reference, which stops at the rows
// and the .matrix file).  DESIGN.md section 2.12 states the algorithm; the host side is tree_average in engine_graph.hip.
//
//   k_tree_check   a row identity outside (0, 100] (NaN included) sets a flag
//   (k_cluster_keys and the stable radix sort of the keys: the rows of a pair adjacent, in the order given — cluster.hpp)
//   k_tree_fill    the dense matrix D (n rows of ld floats, ld = n rounded up to 64): d_missing, +inf on the diagonal and in the padding
//   k_tree_fold    per pair, cluster_fold_at's w -> d = 1 - w / 100 into D[lo][hi] and D[hi][lo]
//   k_tree_rowmin  per row k, its minimum (D[k][j], j) as one row key; sizes, ids and active flags set
//   k_tree_first   the pick of merge 0 (one workgroup)
//   k_tree_merge   one launch per merge: merges the picked pair, keeps the row minima and picks the next pair (its last workgroup)
//
// Distances are non-negative floats or +inf, so their bit patterns order like their values and a lexicographic minimum is a minimum
// of 64-bit keys: a row key is bits(d) << 32 | column, a pair key bits(d) << 32 | lo << 16 | hi (ids below 2^16).  A retired column
// holds +inf in every active row, so a row scan needs no active flags.  Each row caches its minimum over the active columns; the
// global pick is the smallest pair key over the row minima, which is rule 4's tie order: the winning pair is row lo's own minimum.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "cluster.hpp"

namespace ani {

constexpr int kTreeRows = 64;                          // rows of D owned by one workgroup of k_tree_merge
constexpr uint32_t kTreeInfBits = 0x7f800000u;         // +inf

__device__ __forceinline__ uint64_t tree_row_key(uint32_t dBits, uint32_t col) { return ((uint64_t)dBits << 32) | col; }
__device__ __forceinline__ uint64_t tree_row_key(float d, uint32_t col) { return tree_row_key(__float_as_uint(d), col); }
// the pair key of row k's minimum
__device__ __forceinline__ uint64_t tree_pair_key(uint64_t rowKey, uint32_t k)
{
  const uint32_t c = (uint32_t)rowKey;
  return (rowKey & 0xffffffff00000000ull) | ((uint64_t)(k < c ? k : c) << 16) | (k < c ? c : k);
}
__device__ __forceinline__ uint64_t tree_min(uint64_t x, uint64_t y) { return x < y ? x : y; }

// d of a pair with rows: (float)(1 - (double)w / 100)
__device__ __forceinline__ float tree_leaf_distance(float w) { return (float)(1.0 - (double)w / 100.0); }
// The average of a merged cluster.  na * x and nb * y are exact in double (a 24-bit mantissa times a count below 2^17), so a
// contraction of the sum into an FMA cannot change the result.
__device__ __forceinline__ float tree_average(float x, float y, double na, double nb) { return (float)((na * (double)x + nb * (double)y) / (na + nb)); }

// smallest key of the workgroup, in every lane; `red` holds kTPB / kWave keys of LDS
__device__ __forceinline__ uint64_t tree_block_min(uint64_t v, uint64_t *red)
{
  for (int d = kWave / 2; d >= 1; d /= 2) v = tree_min(v, __shfl_xor(v, d));
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  block_barrier();
  v = red[0];
  for (int w = 1; w < kTPB / kWave; w++) v = tree_min(v, red[w]);
  block_barrier();                                       // red is free again
  return v;
}

// row minimum over all ld columns (the diagonal, retired columns and the padding hold +inf), by the whole workgroup
__device__ __forceinline__ uint64_t tree_scan_row(const float *row, uint64_t ld, uint64_t *red)
{
  const uint4 *r4 = (const uint4 *)row;
  uint64_t best = ~0ull;
#pragma unroll 4
  for (uint32_t q = threadIdx.x; q < (uint32_t)(ld / 4); q += kTPB) {
    const uint4 v = r4[q];
    const uint32_t j = 4 * q;
    best = tree_min(best, tree_min(tree_min(tree_row_key(v.x, j), tree_row_key(v.y, j + 1)), tree_min(tree_row_key(v.z, j + 2), tree_row_key(v.w, j + 3))));
  }
  return tree_block_min(best, red);
}

struct TreeArgs {
  float *D; uint64_t ld; int32_t n;
  uint64_t *rowMin;                                      // per row: row key of its minimum over the active columns
  int32_t *size, *id;                                    // per slot: cluster size, cluster id (leaf i, or n + s for merge s)
  uint32_t *active;
  int32_t *pick;                                         // the merge to do next: {a, b, na, nb}
  uint64_t *part;                                        // per workgroup of k_tree_merge: {best pair key of its rows, best row key of row a in its columns}
  uint32_t *arrived;                                     // workgroups of k_tree_merge arrived, summed over the launches
  int32_t *children; float *height;                      // the result, 2 ids and a height per merge
};

// One thread: record merge `step` (the pair of `best`) and make it the next merge: slot lo takes the cluster, hi is retired.
__device__ __forceinline__ void tree_pick(const TreeArgs &t, uint64_t best, int32_t step)
{
  const int32_t lo = (int32_t)((best >> 16) & 0xffffu), hi = (int32_t)(best & 0xffffu);
  const int32_t ia = t.id[lo], ib = t.id[hi], na = t.size[lo], nb = t.size[hi];
  t.children[2 * step] = ia < ib ? ia : ib;
  t.children[2 * step + 1] = ia < ib ? ib : ia;
  t.height[step] = __uint_as_float((uint32_t)(best >> 32));
  t.pick[0] = lo; t.pick[1] = hi; t.pick[2] = na; t.pick[3] = nb;
  t.id[lo] = t.n + step; t.size[lo] = na + nb; t.active[hi] = 0u;
}

// Workgroup arrival of the "last workgroup finishes the reduction" hand-off (the agent-scope release / acquire pair of the counter
// recipe): only the calling lane stored what is handed off.
__device__ __forceinline__ uint32_t tree_arrive(uint32_t *counter)
{
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return atomicAdd(counter, 1u);
#endif
}
__device__ __forceinline__ void tree_acquire()
{
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

static __global__ void k_tree_check(const ani_cgi_t *__restrict__ rows, uint64_t n, uint32_t *__restrict__ bad)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = rows[i].identity;
  if (!(x > 0.0f && x <= 100.0f)) atomicOr(bad, 2u);
}

// one workgroup per row
static __global__ __launch_bounds__(kTPB) void k_tree_fill(float *__restrict__ D, uint64_t ld, int32_t n, float dMissing)
{
  const uint32_t k = blockIdx.x;
  uint4 *r4 = (uint4 *)(D + (uint64_t)k * ld);
  const uint32_t miss = __float_as_uint(dMissing);
  for (uint32_t q = threadIdx.x; q < (uint32_t)(ld / 4); q += kTPB) {
    uint32_t v[4];
    for (int e = 0; e < 4; e++) { const uint32_t j = 4 * q + e; v[e] = (j == k || j >= (uint32_t)n) ? kTreeInfBits : miss; }
    uint4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    r4[q] = o;
  }
}

static __global__ void k_tree_fold(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                   uint64_t n, int b, float *__restrict__ D, uint64_t ld)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t lo, hi; float w;
  if (i >= n || !cluster_fold_at(keys, vals, rows, n, i, b, &lo, &hi, &w)) return;
  const float d = tree_leaf_distance(w);
  D[(uint64_t)lo * ld + hi] = d;
  D[(uint64_t)hi * ld + lo] = d;
}

// one workgroup per row
static __global__ __launch_bounds__(kTPB) void k_tree_rowmin(TreeArgs t)
{
  __shared__ uint64_t red[kTPB / kWave];
  const uint32_t k = blockIdx.x;
  const uint64_t m = tree_scan_row(t.D + (uint64_t)k * t.ld, t.ld, red);
  if (threadIdx.x == 0) { t.rowMin[k] = m; t.size[k] = 1; t.id[k] = (int32_t)k; t.active[k] = 1u; }
}

// one workgroup: the first pick (n >= 2)
static __global__ __launch_bounds__(kTPB) void k_tree_first(TreeArgs t)
{
  __shared__ uint64_t red[kTPB / kWave];
  uint64_t best = ~0ull;
  for (uint32_t k = threadIdx.x; k < (uint32_t)t.n; k += kTPB) best = tree_min(best, tree_pair_key(t.rowMin[k], k));
  best = tree_block_min(best, red);
  if (threadIdx.x == 0) tree_pick(t, best, 0);
}

// Merge s: cluster b goes into slot a.  Workgroup g owns rows [64 g, 64 g + 64): one lane per row computes the new d(k, a), writes it
// to D[k][a] and D[a][k] and +inf to D[k][b], and updates the row's cached minimum (m, c), which can only rise if c was a or b:
//   - (c == a or b) and d(k, a) > m: the row is rescanned, by the whole workgroup, after the barrier;
//   - otherwise the minimum is the smaller of (m, c) and (d(k, a), a): an unchanged value at b moves to a, an equal one at c > a too.
// Row a's new minimum is the smallest (d(k, a), k): each workgroup reduces its columns, and the last workgroup to arrive combines
// those with the pair keys of every other row into the pick of merge s + 1.
static __global__ __launch_bounds__(kTPB) void k_tree_merge(TreeArgs t, int32_t s)
{
  __shared__ uint64_t red[kTPB / kWave];
  __shared__ uint32_t list[kTreeRows];
  __shared__ uint32_t nList, last;
  const uint32_t a = (uint32_t)t.pick[0], b = (uint32_t)t.pick[1];
  const double na = (double)t.pick[2], nb = (double)t.pick[3];
  const uint32_t tid = threadIdx.x, k = blockIdx.x * kTreeRows + tid;
  if (tid == 0) nList = 0;
  block_barrier();
  uint64_t keyK = ~0ull, keyA = ~0ull;
  if (tid < (uint32_t)kTreeRows && k < (uint32_t)t.n) {
    if (k == b) t.D[(uint64_t)a * t.ld + b] = __uint_as_float(kTreeInfBits);
    else if (k != a && t.active[k]) {
      float *row = t.D + (uint64_t)k * t.ld;
      const float dn = tree_average(row[a], row[b], na, nb);
      row[a] = dn; row[b] = __uint_as_float(kTreeInfBits);
      t.D[(uint64_t)a * t.ld + k] = dn;
      keyA = tree_row_key(dn, k);
      uint64_t m = t.rowMin[k];
      const uint32_t c = (uint32_t)m;
      if ((c == a || c == b) && __float_as_uint(dn) > (uint32_t)(m >> 32)) list[atomicAdd(&nList, 1u)] = k;
      else {
        const uint64_t cand = tree_row_key(dn, a);
        if (cand < m) { m = cand; t.rowMin[k] = m; }
        keyK = tree_pair_key(m, k);
      }
    }
  }
  block_barrier_mem();                                   // the rows' new column a and +inf in column b are stored before the rescans read them
  const uint32_t nl = nList;
  for (uint32_t r = 0; r < nl; r++) {
    const uint32_t kr = list[r];
    const uint64_t m = tree_scan_row(t.D + (uint64_t)kr * t.ld, t.ld, red);
    if (tid == 0) t.rowMin[kr] = m;
    if (k == kr) keyK = tree_pair_key(m, kr);
  }
  if (s + 1 > t.n - 2) return;                           // the last merge: nothing left to pick
  keyK = tree_block_min(keyK, red);
  keyA = tree_block_min(keyA, red);
  if (tid == 0) {
    t.part[2 * blockIdx.x] = keyK;
    t.part[2 * blockIdx.x + 1] = keyA;
    last = tree_arrive(t.arrived) == (uint32_t)(s + 1) * gridDim.x - 1u;
    if (last) tree_acquire();
  }
  block_barrier();
  if (!last) return;
  keyK = ~0ull; keyA = ~0ull;
  for (uint32_t g = tid; g < gridDim.x; g += kTPB) { keyK = tree_min(keyK, t.part[2 * g]); keyA = tree_min(keyA, t.part[2 * g + 1]); }
  keyK = tree_block_min(keyK, red);
  keyA = tree_block_min(keyA, red);
  if (tid == 0) {
    t.rowMin[a] = keyA;
    tree_pick(t, tree_min(keyK, tree_pair_key(keyA, a)), s + 1);
  }
}

}  // namespace ani
