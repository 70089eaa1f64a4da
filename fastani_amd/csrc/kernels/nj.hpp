// nj.hpp — neighbour-joining tree of the genomes (ani_tree_nj; no counterpart in the reference, which stops at the rows and the
// .matrix file).  include/ani_abi.h states the semantics, DESIGN.md section 2.13 the algorithm; the host side is tree_nj in engine_graph.hip.
//
//   (k_tree_check, k_cluster_keys and the stable radix sort of the keys: as for the average-linkage tree — tree.hpp, cluster.hpp)
//   k_nj_fill      the dense matrix q (n rows of ld int32, ld = n rounded up to 64): q_missing, the sentinel on the diagonal and in the padding
//   k_nj_fold      per pair, cluster_fold_at's w -> nj_leaf_distance(w) into q[lo][hi] and q[hi][lo]
//   k_nj_rowsum    per row k, R[k] = the sum of its cells; ids and active flags set
//   k_nj_scan      one launch per record: the smallest Q(a, b) = (m - 2) q(a, b) - R[a] - R[b] over the upper triangle; its last
//                  workgroup writes record s and the pick of join s
//   k_nj_update    join s: row / column a take the new node, row / column b the sentinel, every R[k] follows
//   k_nj_map, k_nj_compact   the active positions, in their order, into a smaller matrix (the host does this whenever an eighth of
//                  the positions is retired, so that a scan reads little more than the active cells)
//
// Everything is integer: sums and Q are exact, so any reduction order gives the same tree.  A cell that takes no part (diagonal,
// padding, retired row or column) holds kNjNone = INT32_MIN, which no distance can be (they are clamped to +-(2^31 - 1)); the scan
// skips it, so it needs no active flags.  Positions keep the order of the slots (the compaction is stable), so "smallest position"
// is rule 4's "smallest slot".
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "cluster.hpp"
#include "tree.hpp"

namespace ani {

constexpr int32_t kNjNone = INT32_MIN;
constexpr int kNjCols = 4 * kWave;                       // columns of a scan tile: one wave wide, 16 bytes per lane
constexpr int64_t kNjWorst = INT64_MAX;

// q of a pair: rint((100 - w) 2^24 / 100), round-half-even; the difference and the product are exact in double
__device__ __forceinline__ int32_t nj_leaf_distance(float w) { return (int32_t)rint((100.0 - (double)w) * 16777216.0 / 100.0); }
// q of the new node to k: floor((x + y - qab) / 2), clamped
__device__ __forceinline__ int32_t nj_joined(int32_t x, int32_t y, int32_t qab)
{
  const int64_t v = ((int64_t)x + (int64_t)y - (int64_t)qab) >> 1;
  return (int32_t)(v > 2147483647ll ? 2147483647ll : (v < -2147483647ll ? -2147483647ll : v));
}

struct NjArgs {
  int32_t *q; uint64_t ld;                               // the matrix: cur rows of ld cells
  int32_t n, cur;                                        // genomes; positions of the matrix (active and retired)
  int64_t *R;                                            // per position: the sum of its row (ld entries, 0 in the padding)
  int32_t *id;                                           // per position: node id (leaf i, or n + s for join s)
  uint32_t *active;
  int32_t *pick;                                         // the join to do next: {a, b, q(a, b)}
  int64_t *partQ; uint32_t *partAB;                      // per workgroup of k_nj_scan: its best Q and pair (a << 16 | b)
  uint32_t *arrived;                                     // workgroups of k_nj_scan arrived (the last one resets it)
  int32_t *children; float *length;                      // the result, 2 ids and 2 lengths per record
};

// the better of two candidates (Q, a << 16 | b): the smaller Q, then the smaller a, then the smaller b
__device__ __forceinline__ bool nj_better(int64_t q, uint32_t ab, int64_t bq, uint32_t bab) { return q < bq || (q == bq && ab < bab); }

__device__ __forceinline__ void nj_wave_min(int64_t &q, uint32_t &ab)
{
  for (int d = kWave / 2; d >= 1; d /= 2) {
    const int64_t oq = __shfl_xor(q, d); const uint32_t oab = __shfl_xor(ab, d);
    if (nj_better(oq, oab, q, ab)) { q = oq; ab = oab; }
  }
}
// the best of the workgroup, in every lane
__device__ __forceinline__ void nj_block_min(int64_t &q, uint32_t &ab, int64_t *redQ, uint32_t *redAB)
{
  nj_wave_min(q, ab);
  if ((threadIdx.x & (kWave - 1)) == 0) { redQ[threadIdx.x / kWave] = q; redAB[threadIdx.x / kWave] = ab; }
  block_barrier();
  q = redQ[0]; ab = redAB[0];
  for (int w = 1; w < kTPB / kWave; w++) if (nj_better(redQ[w], redAB[w], q, ab)) { q = redQ[w]; ab = redAB[w]; }
  block_barrier();                                       // the arrays are free again
}

// one workgroup per row
static __global__ __launch_bounds__(kTPB) void k_nj_fill(int32_t *__restrict__ q, uint64_t ld, int32_t n, int32_t qMissing)
{
  const uint32_t k = blockIdx.x;
  uint4 *r4 = (uint4 *)(q + (uint64_t)k * ld);
  for (uint32_t p = threadIdx.x; p < (uint32_t)(ld / 4); p += kTPB) {
    int32_t v[4];
    for (int e = 0; e < 4; e++) { const uint32_t j = 4 * p + e; v[e] = (j == k || j >= (uint32_t)n) ? kNjNone : qMissing; }
    uint4 o; o.x = (uint32_t)v[0]; o.y = (uint32_t)v[1]; o.z = (uint32_t)v[2]; o.w = (uint32_t)v[3];
    r4[p] = o;
  }
}

static __global__ void k_nj_fold(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const ani_cgi_t *__restrict__ rows,
                                 uint64_t n, int b, int32_t *__restrict__ q, uint64_t ld)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t lo, hi; float w;
  if (i >= n || !cluster_fold_at(keys, vals, rows, n, i, b, &lo, &hi, &w)) return;
  const int32_t d = nj_leaf_distance(w);
  q[(uint64_t)lo * ld + hi] = d;
  q[(uint64_t)hi * ld + lo] = d;
}

// one workgroup per row of the first matrix (grid = ld: the padding's R is 0)
static __global__ __launch_bounds__(kTPB) void k_nj_rowsum(NjArgs t)
{
  __shared__ int64_t red[kTPB / kWave];
  const uint32_t k = blockIdx.x;
  int64_t sum = 0;
  if (k < (uint32_t)t.n) {
    const uint4 *r4 = (const uint4 *)(t.q + (uint64_t)k * t.ld);
    for (uint32_t p = threadIdx.x; p < (uint32_t)(t.ld / 4); p += kTPB) {
      const uint4 v = r4[p];
      const int32_t x[4] = {(int32_t)v.x, (int32_t)v.y, (int32_t)v.z, (int32_t)v.w};
      for (int e = 0; e < 4; e++) sum += x[e] == kNjNone ? 0 : (int64_t)x[e];
    }
  }
  for (int d = kWave / 2; d >= 1; d /= 2) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = sum;
  block_barrier();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kTPB / kWave; w++) sum += red[w];
    t.R[k] = sum;
    if (k < (uint32_t)t.n) { t.id[k] = (int32_t)k; t.active[k] = 1u; }
  }
}

// One wave over the rows r0 + wave, r0 + wave + 4, ... < r1 of a tile, columns c .. c + 3 in this lane (negR: minus their R).
// DIAG: the tile touches the diagonal, only cells with column > row count.
template <bool DIAG>
__device__ __forceinline__ void nj_scan_rows(const NjArgs &t, int64_t mul, uint32_t r0, uint32_t r1, uint32_t c, const int64_t (&negR)[4],
                                             int64_t &best, uint32_t &bestAB)
{
#pragma unroll 4
  for (uint32_t r = r0 + threadIdx.x / kWave; r < r1; r += kTPB / kWave) {
    const uint4 v = *(const uint4 *)(t.q + (uint64_t)r * t.ld + c);
    const int64_t nr = -t.R[r];
    const int32_t x[4] = {(int32_t)v.x, (int32_t)v.y, (int32_t)v.z, (int32_t)v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int64_t Q = mul * (int64_t)x[e] + negR[e] + nr;
      const bool ok = x[e] != kNjNone && (!DIAG || c + e > r);
      if (ok && Q < best) { best = Q; bestAB = (r << 16) | (c + e); }    // rows and columns ascend: the first of equal ones stays
    }
  }
}

// One thread: record s from the best pair.  s < n - 2: a join (rule 5), which becomes the pick; s = n - 2: the last two nodes (rule 7).
__device__ __forceinline__ void nj_record(const NjArgs &t, uint32_t ab, int32_t s)
{
  const uint32_t a = ab >> 16, b = ab & 0xffffu;
  if (a >= b || b >= (uint32_t)t.cur) return;            // (no candidate: cannot happen with two active positions)
  const int32_t m = t.n - s, qab = t.q[(uint64_t)a * t.ld + b];
  double la = (double)qab, lb = (double)qab;
  if (m > 2) {
    const double d = (double)(t.R[a] - t.R[b]) / (double)(m - 2);
    la += d; lb -= d;
  }
  const float fa = (float)(la * 0.5 / 16777216.0), fb = (float)(lb * 0.5 / 16777216.0);
  const int32_t ia = t.id[a], ib = t.id[b];
  t.children[2 * s] = ia < ib ? ia : ib; t.children[2 * s + 1] = ia < ib ? ib : ia;
  t.length[2 * s] = ia < ib ? fa : fb; t.length[2 * s + 1] = ia < ib ? fb : fa;
  if (m > 2) {
    t.pick[0] = (int32_t)a; t.pick[1] = (int32_t)b; t.pick[2] = qab;
    t.id[a] = t.n + s; t.active[b] = 0u; t.R[a] = 0;               // k_nj_update adds the new row's cells to R[a]
  }
}

// Record s.  Tiles of rowsPerTile rows x kNjCols columns, row-major; workgroup g takes the tiles g, g + gridDim.x, ... that reach
// above the diagonal.  A lane keeps the R of its four columns in registers down the rows of a tile, a wave reads 1 KiB of a row at a
// time.  The last workgroup to arrive reduces the workgroups' candidates and writes the record.
static __global__ __launch_bounds__(kTPB) void k_nj_scan(NjArgs t, int32_t s, uint32_t rowsPerTile)
{
  __shared__ int64_t redQ[kTPB / kWave];
  __shared__ uint32_t redAB[kTPB / kWave];
  __shared__ uint32_t last;
  const uint32_t cur = (uint32_t)t.cur, lane = threadIdx.x & (kWave - 1);
  const uint32_t nCT = (cur + kNjCols - 1) / kNjCols, nRT = (cur + rowsPerTile - 1) / rowsPerTile;
  const int64_t mul = (int64_t)(t.n - s - 2);
  int64_t best = kNjWorst; uint32_t bestAB = ~0u;
  for (uint32_t tile = blockIdx.x; tile < nCT * nRT; tile += gridDim.x) {
    const uint32_t r0 = (tile / nCT) * rowsPerTile, c0 = (tile % nCT) * kNjCols;
    if (c0 + kNjCols - 1 <= r0) continue;                 // below the diagonal
    const uint32_t r1 = r0 + rowsPerTile < cur ? r0 + rowsPerTile : cur, c = c0 + 4 * lane;
    if (c >= (uint32_t)t.ld) continue;                    // (ld is a multiple of 64, not of the tile width)
    int64_t negR[4];
    for (int e = 0; e < 4; e++) negR[e] = -t.R[c + e];
    int64_t tq = kNjWorst; uint32_t tab = ~0u;             // the tile's best: inside a tile a lane's cells come in rule 4's order
    if (c0 < r1) nj_scan_rows<true>(t, mul, r0, r1, c, negR, tq, tab);
    else nj_scan_rows<false>(t, mul, r0, r1, c, negR, tq, tab);
    if (nj_better(tq, tab, best, bestAB)) { best = tq; bestAB = tab; }
  }
  nj_block_min(best, bestAB, redQ, redAB);
  if (threadIdx.x == 0) {
    t.partQ[blockIdx.x] = best; t.partAB[blockIdx.x] = bestAB;
    last = tree_arrive(t.arrived) == gridDim.x - 1u;
    if (last) tree_acquire();
  }
  block_barrier();
  if (!last) return;
  best = kNjWorst; bestAB = ~0u;
  for (uint32_t g = threadIdx.x; g < gridDim.x; g += kTPB) {
    const int64_t pq = t.partQ[g]; const uint32_t pab = t.partAB[g];
    if (nj_better(pq, pab, best, bestAB)) { best = pq; bestAB = pab; }
  }
  nj_block_min(best, bestAB, redQ, redAB);
  if (threadIdx.x == 0) { *t.arrived = 0u; nj_record(t, bestAB, s); }
}

// Join s of the pick {a, b, qab}, one lane per position k: q(a, k) = q(k, a) = nj_joined(...), q(b, k) = q(k, b) = none, R[k] follows by
// the difference; the new row's sum goes to R[a] (zeroed with the pick), one atomic per workgroup.
static __global__ __launch_bounds__(kTPB) void k_nj_update(NjArgs t)
{
  __shared__ int64_t red[kTPB / kWave];
  const uint32_t a = (uint32_t)t.pick[0], b = (uint32_t)t.pick[1], k = blockIdx.x * kTPB + threadIdx.x;
  const int32_t qab = t.pick[2];
  int32_t *rowA = t.q + (uint64_t)a * t.ld, *rowB = t.q + (uint64_t)b * t.ld;
  int64_t sum = 0;
  if (k == b) { rowA[b] = kNjNone; rowB[a] = kNjNone; }
  else if (k < (uint32_t)t.cur && k != a && t.active[k]) {
    const int32_t x = rowA[k], y = rowB[k], v = nj_joined(x, y, qab);
    int32_t *rowK = t.q + (uint64_t)k * t.ld;
    rowA[k] = v; rowK[a] = v; rowB[k] = kNjNone; rowK[b] = kNjNone;
    t.R[k] += (int64_t)v - (int64_t)x - (int64_t)y;
    sum = v;
  }
  for (int d = kWave / 2; d >= 1; d /= 2) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = sum;
  block_barrier();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kTPB / kWave; w++) sum += red[w];
    if (sum) atomicAdd((unsigned long long *)&t.R[a], (unsigned long long)sum);
  }
}

// One workgroup: newPos[p] = the active positions before p; R, id and the flags of the compacted matrix `to` (to.cur active positions,
// R = 0 in its padding).
static __global__ __launch_bounds__(kTPB) void k_nj_map(NjArgs from, NjArgs to, uint32_t *__restrict__ newPos)
{
  __shared__ uint32_t count[kTPB];
  const uint32_t cur = (uint32_t)from.cur, per = (cur + kTPB - 1) / kTPB;
  const uint32_t p0 = threadIdx.x * per < cur ? threadIdx.x * per : cur, p1 = p0 + per < cur ? p0 + per : cur;
  uint32_t c = 0;
  for (uint32_t p = p0; p < p1; p++) c += from.active[p] ? 1u : 0u;
  count[threadIdx.x] = c;
  block_barrier();
  uint32_t at = 0;
  for (uint32_t i = 0; i < threadIdx.x; i++) at += count[i];
  for (uint32_t p = p0; p < p1; p++) {
    newPos[p] = at;
    if (from.active[p]) { to.R[at] = from.R[p]; to.id[at] = from.id[p]; to.active[at] = 1u; at++; }
  }
  for (uint32_t p = (uint32_t)to.cur + threadIdx.x; p < (uint32_t)to.ld; p += kTPB) to.R[p] = 0;
}

// one workgroup per row of `from`: an active row's active cells go to their new places, the padding of the new row is none
static __global__ __launch_bounds__(kTPB) void k_nj_compact(NjArgs from, NjArgs to, const uint32_t *__restrict__ newPos)
{
  const uint32_t r = blockIdx.x;
  if (!from.active[r]) return;
  const int32_t *src = from.q + (uint64_t)r * from.ld;
  int32_t *dst = to.q + (uint64_t)newPos[r] * to.ld;
  for (uint32_t c = threadIdx.x; c < (uint32_t)from.cur; c += kTPB) if (from.active[c]) dst[newPos[c]] = src[c];
  for (uint32_t c = (uint32_t)to.cur + threadIdx.x; c < (uint32_t)to.ld; c += kTPB) dst[c] = kNjNone;
}

}  // namespace ani
