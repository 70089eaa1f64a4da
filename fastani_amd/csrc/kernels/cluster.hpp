// cluster.hpp — greedy ANI clustering of the pair graph (ani_cluster_greedy; no counterpart in the reference, which stops at the
// rows and the .matrix file).  DESIGN.md section 2.11 states the algorithm; the host side is cluster_greedy in engine_graph.hip.
//
//   k_cluster_keys     row -> key min << b | max (b = bit width of the genome ids) and its position; ids checked
//   (stable radix sort of the keys: the rows of one pair end up adjacent, in the order they were given)
//   k_cluster_fold     per key segment, in order: first row sets w, every later one w = (w + id) / 2 (float); w >= T -> an edge
//   k_cluster_degrees  lower + upper degree per vertex (the prefix sum over it gives the CSR offsets), fill cursors zeroed
//   k_cluster_scatter  both directions of every edge into the CSR: a vertex's lower neighbours first, then its upper ones
//   k_cluster_round    one round of the greedy: an undecided vertex becomes a member as soon as a lower neighbour is a
//                      representative, a representative once every lower neighbour is a member
//   k_cluster_assign   member -> the adjacent representative with the largest w (ties: the smallest id)
//
// State words (one per vertex) change at most once, from undecided to representative or member, and only their owner lane writes
// them.  They are read and written with relaxed agent-scope atomics: a reader that sees a stale "undecided" only decides later, so
// a round reproduces the sequential greedy whatever it observes of the others.  Visibility across workgroups comes from the kernel
// boundaries; inside a workgroup the round repeats (barrier to barrier) while it still decides something, which resolves chains of
// consecutive vertices — an ordered path — inside one launch.  A vertex with more than kClusterWaveDeg neighbours to scan is
// scanned by its whole wave.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"

namespace ani {

constexpr uint32_t kClusterUndecided = 0, kClusterRep = 1, kClusterMember = 2, kClusterNone = 3;
constexpr uint32_t kClusterWaveDeg = 32;

__device__ __forceinline__ uint32_t cluster_state_load(const uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *(const volatile uint32_t *)p;
#endif
}
__device__ __forceinline__ void cluster_state_store(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *(volatile uint32_t *)p = v;
#endif
}
__device__ __forceinline__ uint32_t cluster_lane() { return threadIdx.x & (kWave - 1); }
// lanes below this one with their bit set in `mask`
__device__ __forceinline__ uint32_t cluster_rank(unsigned long long mask) { return (uint32_t)__popcll(mask & ((1ull << cluster_lane()) - 1ull)); }

// keys[i] = min(q, r) << b | max(q, r), vals[i] = i; a row with an id outside [0, nGenomes) sets *bad
static __global__ void k_cluster_keys(const ani_cgi_t *__restrict__ rows, uint64_t n, int32_t nGenomes, int b, uint64_t *__restrict__ keys,
                                      uint32_t *__restrict__ vals, uint32_t *__restrict__ bad)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t q = rows[i].qryGenomeId, r = rows[i].refGenomeId;
  if (q < 0 || q >= nGenomes || r < 0 || r >= nGenomes) { atomicOr(bad, 1u); keys[i] = 0; vals[i] = (uint32_t)i; return; }
  const uint32_t lo = (uint32_t)(q < r ? q : r), hi = (uint32_t)(q < r ? r : q);
  keys[i] = ((uint64_t)lo << b) | hi;
  vals[i] = (uint32_t)i;
}

// The pair value at sorted position i (i < n): true at the first position of a key that is not a self pair, with the pair {lo < hi}
// and its rows folded in their order (the first sets w, every later one w = (w + id) / 2 in float); false everywhere else.  Shared
// with the tree (tree.hpp), so that the .clusters and .newick files fold a pair as the .matrix cell does.
__device__ __forceinline__ bool cluster_fold_at(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                                uint64_t n, uint64_t i, int b, uint32_t *lo, uint32_t *hi, float *w)
{
  const uint64_t key = keys[i];
  if (i != 0 && keys[i - 1] == key) return false;
  *lo = (uint32_t)(key >> b); *hi = (uint32_t)(key & ((1ull << b) - 1ull));
  if (*lo == *hi) return false;                                    // self rows have no pair value
  float x = rows[vals[i]].identity;
  for (uint64_t j = i + 1; j < n && keys[j] == key; j++) x = (x + rows[vals[j]].identity) / 2.0f;
  *w = x;
  return true;
}

// one lane per sorted position; the first position of every key folds the key's rows in their order.  Edges {lo < hi, w} go to
// a compacted list (one cursor bump per wave) and count towards lowDeg[hi] / highDeg[lo].
static __global__ void k_cluster_fold(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                      uint64_t n, int b, float minIdentity, uint32_t *__restrict__ edgeCount, int32_t *__restrict__ eLo,
                                      int32_t *__restrict__ eHi, float *__restrict__ eW, int32_t *__restrict__ lowDeg, int32_t *__restrict__ highDeg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool edge = false; uint32_t lo = 0, hi = 0; float w = 0.0f;
  if (i < n && cluster_fold_at(keys, vals, rows, n, i, b, &lo, &hi, &w)) edge = w >= minIdentity;
  const unsigned long long m = __ballot(edge);
  if (!m) return;
  uint32_t base = 0;
  if (cluster_lane() == (uint32_t)(__ffsll(m) - 1)) base = atomicAdd(edgeCount, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, __ffsll(m) - 1);
  if (edge) {
    const uint32_t e = base + cluster_rank(m);
    eLo[e] = (int32_t)lo; eHi[e] = (int32_t)hi; eW[e] = w;
    atomicAdd(&lowDeg[hi], 1); atomicAdd(&highDeg[lo], 1);
  }
}

static __global__ void k_cluster_degrees(int32_t nV, const int32_t *__restrict__ lowDeg, const int32_t *__restrict__ highDeg,
                                         int32_t *__restrict__ deg, int32_t *__restrict__ fill)
{
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  deg[v] = lowDeg[v] + highDeg[v];
  fill[2 * v] = 0; fill[2 * v + 1] = 0;
}

// adjacency of v: [off[v], off[v] + lowDeg[v]) the lower neighbours, then the upper ones (in no particular order)
static __global__ void k_cluster_scatter(uint32_t nE, const int32_t *__restrict__ eLo, const int32_t *__restrict__ eHi, const float *__restrict__ eW,
                                         const uint32_t *__restrict__ off, const int32_t *__restrict__ lowDeg, int32_t *__restrict__ fill,
                                         int32_t *__restrict__ nbr, float *__restrict__ nbrW)
{
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nE) return;
  const int32_t lo = eLo[e], hi = eHi[e]; const float w = eW[e];
  const uint32_t a = off[hi] + (uint32_t)atomicAdd(&fill[2 * hi], 1);
  nbr[a] = lo; nbrW[a] = w;
  const uint32_t c = off[lo] + (uint32_t)lowDeg[lo] + (uint32_t)atomicAdd(&fill[2 * lo + 1], 1);
  nbr[c] = hi; nbrW[c] = w;
}

// One round over the vertices of each workgroup (one lane per vertex), repeated inside the workgroup while it decides something.
// `undecided` (optional): vertices still undecided at the end, summed over the grid.
static __global__ __launch_bounds__(kTPB) void k_cluster_round(int32_t nV, const uint32_t *__restrict__ off, const int32_t *__restrict__ lowDeg,
                                                               const int32_t *__restrict__ nbr, uint32_t *state, uint32_t *undecided)
{
  __shared__ uint32_t stamp[2];
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = cluster_lane();
  uint32_t s = v < nV ? cluster_state_load(&state[v]) : kClusterNone;
  const uint32_t o = v < nV ? off[v] : 0u, cnt = v < nV ? (uint32_t)lowDeg[v] : 0u;
  if (threadIdx.x == 0) { stamp[0] = 0; stamp[1] = 0; }
  __syncthreads();
  for (uint32_t it = 0;; it++) {
    const bool und = s == kClusterUndecided;
    uint32_t dec = kClusterUndecided;
    if (und && cnt <= kClusterWaveDeg) {
      bool anyU = false, anyR = false;
      for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t t = cluster_state_load(&state[nbr[o + k]]);
        if (t == kClusterRep) { anyR = true; break; }
        anyU |= t == kClusterUndecided;
      }
      dec = anyR ? kClusterMember : (anyU ? kClusterUndecided : kClusterRep);
    }
    // long lists: the whole wave scans one vertex's lower neighbours at a time
    for (unsigned long long big = __ballot(und && cnt > kClusterWaveDeg); big; big &= big - 1) {
      const int l = __ffsll(big) - 1;
      const uint32_t bo = (uint32_t)__shfl((int)o, l), bc = (uint32_t)__shfl((int)cnt, l);
      bool anyU = false, anyR = false;
      for (uint32_t k0 = 0; k0 < bc; k0 += kWave) {
        const uint32_t k = k0 + lane;
        const uint32_t t = k < bc ? cluster_state_load(&state[nbr[bo + k]]) : kClusterMember;
        if (__ballot(t == kClusterRep)) { anyR = true; break; }
        anyU |= __ballot(t == kClusterUndecided) != 0;
      }
      if (lane == (uint32_t)l) dec = anyR ? kClusterMember : (anyU ? kClusterUndecided : kClusterRep);
    }
    if (dec != kClusterUndecided) { s = dec; cluster_state_store(&state[v], dec); stamp[it & 1] = it + 1; }
    __syncthreads();
    const bool again = stamp[it & 1] == it + 1;                 // (the other slot is written only after the next barrier)
    if (!again) break;
  }
  if (undecided) {
    const unsigned long long m = __ballot(s == kClusterUndecided);
    if (m && lane == 0) atomicAdd(undecided, (uint32_t)__popcll(m));
  }
}

// the better of two candidates (w, r): larger w, then smaller r (r < 0: none)
__device__ __forceinline__ bool cluster_better(float w, int32_t r, float bw, int32_t br) { return r >= 0 && (br < 0 || w > bw || (w == bw && r < br)); }

static __global__ __launch_bounds__(kTPB) void k_cluster_assign(int32_t nV, const uint32_t *__restrict__ off, const int32_t *__restrict__ nbr,
                                                                const float *__restrict__ nbrW, const uint32_t *state, int32_t *__restrict__ rep,
                                                                float *__restrict__ repW)
{
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = cluster_lane();
  const uint32_t s = v < nV ? cluster_state_load(&state[v]) : kClusterNone;
  const uint32_t o = v < nV ? off[v] : 0u, cnt = v < nV ? off[v + 1] - o : 0u;
  const bool member = s == kClusterMember;
  float bw = 0.0f; int32_t br = -1;
  if (member && cnt <= kClusterWaveDeg)
    for (uint32_t k = 0; k < cnt; k++) {
      const int32_t r = nbr[o + k];
      if (cluster_state_load(&state[r]) != kClusterRep) continue;
      const float w = nbrW[o + k];
      if (cluster_better(w, r, bw, br)) { bw = w; br = r; }
    }
  for (unsigned long long big = __ballot(member && cnt > kClusterWaveDeg); big; big &= big - 1) {
    const int l = __ffsll(big) - 1;
    const uint32_t bo = (uint32_t)__shfl((int)o, l), bc = (uint32_t)__shfl((int)cnt, l);
    float lw = 0.0f; int32_t lr = -1;
    for (uint32_t k = lane; k < bc; k += kWave) {
      const int32_t r = nbr[bo + k];
      if (cluster_state_load(&state[r]) != kClusterRep) continue;
      const float w = nbrW[bo + k];
      if (cluster_better(w, r, lw, lr)) { lw = w; lr = r; }
    }
    for (int d = kWave / 2; d >= 1; d /= 2) {
      const float ow = __shfl_xor(lw, d); const int32_t orr = __shfl_xor(lr, d);
      if (cluster_better(ow, orr, lw, lr)) { lw = ow; lr = orr; }
    }
    if (lane == (uint32_t)l) { bw = lw; br = lr; }
  }
  if (v >= nV) return;
  if (s == kClusterRep) { rep[v] = v; repW[v] = 0.0f; }
  else { rep[v] = br; repW[v] = bw; }                          // a member always has a representative neighbour
}

}  // namespace ani
