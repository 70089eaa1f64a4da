// single.hpp — single-linkage tree of the genomes = the minimum spanning forest of the pair graph (ani_tree_single; no counterpart in the
// reference, which stops at the rows and the .matrix file).  DESIGN.md section 2.15 states the algorithm; the host side is tree_single
// in engine_graph.hip.
//
//   (k_tree_check, k_cluster_keys and the stable radix sort of the keys: the rows of a pair adjacent, in the order given)
//   k_single_flag     per sorted position: 1 where a pair starts whose folded d lies below d_missing (an edge), else 0
//   (device_scan of the flags: the edges keep their (lo, hi) order)
//   k_single_pairs    the edges, compacted: lo, hi, and bits(d) as the key of the second sort with the edge's position as its payload
//   (stable radix sort over the 32 bits of d: position r of the result is the edge of rank r in the order (bits(d), lo, hi))
//   k_single_rank     lo, hi, bits(d) and a source byte of every edge by rank: a ranked edge list
//   (the forest stage, single_forest in engine_graph.hip, over a ranked edge list:)
//   k_single_init     every vertex its own component, no best edge
//   per round (Boruvka):
//   k_single_best     a live edge whose ends lie in two components offers its rank to both (atomicMin) and stays live
//   k_single_hook     a component root hooks along its best edge; of a mutual pair the root with the larger id; the edge is chosen
//   k_single_jump     every root of the round follows the hooks to the root that remains (compressing as it goes)
//   k_single_label    vertex -> the new root of its old root; best edges cleared
//   (device_scan of the chosen flags)
//   k_single_records  the chosen edges in rank order: the forest, itself a ranked edge list
//
// ani_tree_single_sketch folds further edges into a forest: MSF(A u B) = MSF(MSF(A) u B) under a strict order.
//   k_single_keyflag / k_single_keys  the sorted distinct keys lo << b | hi of the non-self pairs with rows (they mask sketch pairs)
//   k_single_merge    two ranked edge lists with no edge in common -> one: an edge's place is its index plus the edges of the other
//                     list that sort before it (a binary search per lane)
//
// Ranks are a strict total order, so the spanning forest is unique and the chosen flags do not depend on the order in which the
// atomics land or the workgroups run: per round and component, atomicMin leaves the smallest rank among its outgoing live edges,
// whatever the arrival order.  The hooks of a round form no cycle but the mutual pairs (a cycle's smallest edge would be the best
// edge of both its ends), and of a mutual pair exactly one side hooks.  A launch never waits for another workgroup: k_single_hook reads
// `comp` and `best` only (complete since the previous launch) and writes `par` and `chosen`; k_single_jump reads and writes `par`
// alone, and whatever it reads there is an ancestor, the old hook or the final root.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "cluster.hpp"
#include "tree.hpp"

namespace ani {

static __global__ void k_single_flag(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                     uint64_t n, int b, uint32_t dmBits, int32_t *__restrict__ flag)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t lo, hi; float w;
  flag[i] = cluster_fold_at(keys, vals, rows, n, i, b, &lo, &hi, &w) && __float_as_uint(tree_leaf_distance(w)) < dmBits ? 1 : 0;
}

// pos[i]: edges before sorted position i.  dKey / idx are the input of the second sort.
static __global__ void k_single_pairs(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                      uint64_t n, int b, uint32_t dmBits, const uint32_t *__restrict__ pos, uint32_t *__restrict__ eLo,
                                      uint32_t *__restrict__ eHi, uint64_t *__restrict__ dKey, uint32_t *__restrict__ idx)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t lo, hi; float w;
  if (i >= n || !cluster_fold_at(keys, vals, rows, n, i, b, &lo, &hi, &w)) return;
  const uint32_t d = __float_as_uint(tree_leaf_distance(w));
  if (d >= dmBits) return;
  const uint32_t p = pos[i];
  eLo[p] = lo; eHi[p] = hi; dKey[p] = (uint64_t)d; idx[p] = p;
}

static __global__ void k_single_rank(uint32_t nE, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ eLo, const uint32_t *__restrict__ eHi,
                                     const uint64_t *__restrict__ dKey, uint8_t source, uint32_t *__restrict__ uLo, uint32_t *__restrict__ uHi,
                                     uint32_t *__restrict__ uD, uint8_t *__restrict__ uSrc)
{
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nE) return;
  const uint32_t p = idx[r];
  uLo[r] = eLo[p]; uHi[r] = eHi[p]; uD[r] = (uint32_t)dKey[r]; uSrc[r] = source;
}

static __global__ void k_single_init(uint32_t nV, uint32_t *__restrict__ comp, uint32_t *__restrict__ best)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  comp[v] = v; best[v] = kSingleNone;
}

// One lane per live edge (liveIn null: the edges 0..nLive-1 themselves).  `best` only falls during the launch, so an offer that the
// relaxed read already finds beaten needs no atomic: most of a dense component's edges stop there.  The edges that still join two
// components go to liveOut (one cursor bump per wave, in no particular order).
static __global__ void k_single_best(const uint32_t *__restrict__ liveIn, uint32_t nLive, const uint32_t *__restrict__ uLo, const uint32_t *__restrict__ uHi,
                                     const uint32_t *__restrict__ comp, uint32_t *best, uint32_t *__restrict__ liveOut, uint32_t *__restrict__ count)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false; uint32_t e = 0;
  if (t < nLive) {
    e = liveIn ? liveIn[t] : t;
    const uint32_t a = comp[uLo[e]], c = comp[uHi[e]];
    keep = a != c;
    if (keep) {
      if (cluster_state_load(&best[a]) > e) atomicMin(&best[a], e);
      if (cluster_state_load(&best[c]) > e) atomicMin(&best[c], e);
    }
  }
  const unsigned long long m = __ballot(keep);
  if (!m) return;
  uint32_t base = 0;
  if (cluster_lane() == (uint32_t)(__ffsll(m) - 1)) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, __ffsll(m) - 1);
  if (keep) liveOut[base + cluster_rank(m)] = e;
}

// One lane per vertex; only the roots of the round (comp[v] == v) act, and every one of them sets par[v].
static __global__ void k_single_hook(uint32_t nV, const uint32_t *__restrict__ comp, const uint32_t *__restrict__ best, const uint32_t *__restrict__ uLo,
                                     const uint32_t *__restrict__ uHi, uint32_t *__restrict__ par, int32_t *__restrict__ chosen)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV || comp[v] != v) return;
  const uint32_t e = best[v];
  uint32_t p = v;
  if (e != kSingleNone) {
    const uint32_t a = comp[uLo[e]], c = comp[uHi[e]];
    const uint32_t o = a == v ? c : a;
    if (!(best[o] == e && v < o)) { p = o; chosen[e] = 1; }      // of a mutual pair the smaller root stays
  }
  par[v] = p;
}

// The roots of the round: follow the hooks to the root that stays (par[r] == r, which no lane of this launch changes) and point at it.
// Another lane may have shortened a path meanwhile: either value read is an ancestor.  A path has fewer than nV hooks; the bound only
// keeps a broken invariant from spinning (*bad is set, and the host gives up).
static __global__ void k_single_jump(uint32_t nV, const uint32_t *__restrict__ comp, uint32_t *par, uint32_t *__restrict__ bad)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV || comp[v] != v) return;
  uint32_t r = cluster_state_load(&par[v]);
  if (r == v) return;
  uint32_t steps = 0;
  for (uint32_t p; (p = cluster_state_load(&par[r])) != r; r = p)
    if (++steps > nV) { atomicOr(bad, 1u); return; }
  cluster_state_store(&par[v], r);
}

static __global__ void k_single_label(uint32_t nV, uint32_t *__restrict__ comp, const uint32_t *__restrict__ par, uint32_t *__restrict__ best)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  comp[v] = par[comp[v]];
  best[v] = kSingleNone;
}

// pos[r]: chosen edges of smaller rank.
static __global__ void k_single_records(uint32_t nE, const int32_t *__restrict__ chosen, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ uLo,
                                        const uint32_t *__restrict__ uHi, const uint32_t *__restrict__ uD, const uint8_t *__restrict__ uSrc,
                                        uint32_t *__restrict__ fLo, uint32_t *__restrict__ fHi, uint32_t *__restrict__ fD, uint8_t *__restrict__ fSrc)
{
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nE || !chosen[r]) return;
  const uint32_t p = pos[r];
  fLo[p] = uLo[r]; fHi[p] = uHi[r]; fD[p] = uD[r]; fSrc[p] = uSrc[r];
}

// ---- folding further edges into a forest (ani_tree_single_sketch) ----

// per sorted position: 1 where a key starts that is not a self pair
static __global__ void k_single_keyflag(const uint64_t *__restrict__ keys, uint64_t n, int b, int32_t *__restrict__ flag)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  flag[i] = (i == 0 || keys[i - 1] != key) && (key >> b) != (key & ((1ull << b) - 1ull)) ? 1 : 0;
}

static __global__ void k_single_keys(const uint64_t *__restrict__ keys, uint64_t n, const int32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                     uint64_t *__restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[pos[i]] = keys[i];
}

struct SingleList { const uint32_t *lo, *hi, *d; const uint8_t *src; uint32_t n; };

// edges of the ranked list `l` that sort before (d, lo, hi), or at it too if `orEqual`
__device__ __forceinline__ uint32_t single_edges_before(const SingleList &l, uint32_t d, uint32_t lo, uint32_t hi, bool orEqual)
{
  const uint64_t pair = ((uint64_t)lo << 32) | hi;
  uint32_t a = 0, c = l.n;
  while (a < c) {
    const uint32_t mid = a + (c - a) / 2;
    const uint32_t md = l.d[mid];
    const uint64_t mp = ((uint64_t)l.lo[mid] << 32) | l.hi[mid];
    const bool before = md != d ? md < d : (orEqual ? mp <= pair : mp < pair);
    if (before) a = mid + 1; else c = mid;
  }
  return a;
}

// One lane per edge of x, then of y.  The lists share no edge (a sketch edge has no rows and belongs to one strip), so either rule alone
// would do; taking "before" for x and "before or equal" for y keeps the places a permutation whatever the input.
static __global__ void k_single_merge(SingleList x, SingleList y, uint32_t *__restrict__ oLo, uint32_t *__restrict__ oHi, uint32_t *__restrict__ oD,
                                      uint8_t *__restrict__ oSrc)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= x.n + y.n) return;
  const bool first = t < x.n;
  const SingleList &mine = first ? x : y, &other = first ? y : x;
  const uint32_t i = first ? t : t - x.n;
  const uint32_t lo = mine.lo[i], hi = mine.hi[i], d = mine.d[i];
  const uint32_t p = i + single_edges_before(other, d, lo, hi, !first);
  oLo[p] = lo; oHi[p] = hi; oD[p] = d; oSrc[p] = mine.src[i];
}

}  // namespace ani
