// signeigh.hpp — the nearest neighbours of every genome under the whole-genome sketch estimate (ani_signature_neighbors; no counterpart
// in the reference).  DESIGN.md section 2.17 states the algorithm; the host side is signature_neighbors in engine_sig.hip.  The
// signatures are staged by k_sigpair_stage (sigdist.hpp); for the rows [r0, r1) of the pair matrix:
//
//   k_signeigh_merge   the rectangular form of the merge tile: row tiles count from genome r0, column tiles from genome 0, every tile
//                      runs; cell (a, b != a) of an (r1 - r0) x ld strip, shared << 16 | size
//   k_signeigh_select  one workgroup per row a: the k candidates with the largest keys identityBits << 32 | (0xffffffff - b), exactly,
//                      in descending key order -> the row's ani_signeighbor_t records and its count
//
// A cell is a candidate iff shared >= minShared and its identity is at least minIdentity.  The identity bits come from a table the host
// fills with its own double arithmetic, one entry per (shared, size) with 1 <= shared <= size (sigstrip_entry); the device computes no
// logarithm.  Identities are non-negative floats, so their bit patterns order like their values, and the keys of a row are distinct
// (they hold b), so "the k largest" is one set.  The select: a radix select over the 32 identity bits (digits of 11, 11 and 10 bits, an
// LDS histogram per digit, integer LDS atomics) finds the identity t of the k-th largest key and how many cells at t belong to the k;
// one pass then takes every cell above t, in any order, and the first cells at t in ascending b, ranked by a workgroup scan; a sort of
// the at most 1024 keys in LDS orders them.  Nothing depends on the order in which lanes or workgroups run.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "sigdist.hpp"
#include "sigstrip.hpp"

namespace ani {

constexpr int kSigNeighMaxK = 1024;                    // largest k (ani_abi.h): the keys of a row are sorted in LDS
constexpr int kSigNeighBins = 2048;                    // histogram bins of a digit of the select

// One tile: genomes [r0 + T y, r0 + T y + T) against genomes [T x, T x + T).  The 2 T rows go to LDS as in sigpair_tile, lane (i, j)
// merges row i with row T + j.  Rows at or beyond r1 and columns at or beyond n have length 0 and no cell; neither has a == b.
template <int T>
__device__ __forceinline__ void signeigh_tile(uint32_t *tile, int32_t *tileLen, const uint32_t *__restrict__ sig, const int32_t *__restrict__ len, uint32_t n,
    uint32_t r0, uint32_t r1, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  const uint32_t ty = blockIdx.y, tx = blockIdx.x;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t quads = (uint32_t)pitch / 4;
  uint4 *tile4 = (uint4 *)tile;
  for (uint32_t r = 0; r < 2 * T; r++) {
    const uint64_t g = r < (uint32_t)T ? (uint64_t)r0 + (uint64_t)ty * T + r : (uint64_t)tx * T + (r - T);
    const int32_t l = g < (r < (uint32_t)T ? r1 : n) ? len[g] : 0;
    if (tid == 0) tileLen[r] = l;
    const uint4 *src = (const uint4 *)(sig + g * (uint32_t)pitch);
    for (uint32_t q = tid; q < ((uint32_t)l + 3) / 4; q += nt) tile4[r * quads + q] = src[q];
  }
  block_barrier();
  if (tid >= (uint32_t)(T * T)) return;
  const uint32_t i = tid / T, j = tid % T;
  const uint64_t a = (uint64_t)r0 + (uint64_t)ty * T + i, b = (uint64_t)tx * T + j;
  if (a >= r1 || b >= n || a == b) return;
  mat[(a - r0) * ld + b] = sig_merge_rows(tile + i * (uint32_t)pitch, tileLen[i], tile + (T + j) * (uint32_t)pitch, tileLen[T + j], size);
}

template <int T, int WORDS>
static __global__ __launch_bounds__(T * T >= kWave ? T * T : kWave) void k_signeigh_merge(const uint32_t *__restrict__ sig, const int32_t *__restrict__ len,
    uint32_t n, uint32_t r0, uint32_t r1, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[2 * T];
  signeigh_tile<T>(tile, tileLen, sig, len, n, r0, r1, pitch, size, mat, ld);
}

// the identity bits of cell v = row[b] of genome a, if the pair is a candidate.  SELF: the row is genome a's own among the columns, and
// its cell (a, a) was never written; a row of other genomes (sigscreen.hpp: a query against the references) has no such cell.
template <bool SELF>
__device__ __forceinline__ bool signeigh_candidate(const uint32_t *__restrict__ row, uint32_t a, uint32_t b, int32_t minShared, const uint32_t *__restrict__ table,
                                                   uint32_t minBits, uint32_t *id)
{
  if (SELF && b == a) return false;                    // (the one cell of the row that was never written)
  const uint32_t v = row[b], shared = v >> 16, size = v & 0xffffu;
  if ((int32_t)shared < minShared || shared > size) return false;
  *id = table[sigstrip_entry(shared, size)];
  return *id >= minBits;
}

// The select of one row of n cells by one workgroup: the list goes to o[0 .. k) and its length to *cnt.  hist, keys, ws, sel and cursor
// are the workgroup's LDS (kSigNeighBins, kSigNeighMaxK, 8, 2 and 1 entries).  Shared by k_signeigh_select and k_sigscreen_select.
template <bool SELF>
__device__ __forceinline__ void signeigh_select_row(uint32_t *hist, uint64_t *keys, int *ws, uint32_t *sel, uint32_t *cursor, const uint32_t *__restrict__ row,
                                                    uint32_t a, uint32_t n, int32_t minShared, const uint32_t *__restrict__ table, uint32_t minBits, int32_t k,
                                                    uint4 *__restrict__ o, int32_t *__restrict__ cnt)
{
  const uint32_t tid = threadIdx.x;

  // the identity t = prefix of the k-th largest key and `need`, the cells at t among the k; or every candidate, if there are at most k
  uint32_t prefix = 0, mask = 0;
  int need = k;
  bool all = false;
  for (int pass = 0; pass < 3; pass++) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, nb = pass == 2 ? 1024 : 2048;
    for (int i = tid; i < kSigNeighBins; i += kTPB) hist[i] = 0u;
    block_barrier();
    for (uint32_t b = tid; b < n; b += kTPB) {
      uint32_t id;
      if (signeigh_candidate<SELF>(row, a, b, minShared, table, minBits, &id) && (id & mask) == prefix) atomicAdd(&hist[(id >> shift) & (uint32_t)(nb - 1)], 1u);
    }
    block_barrier();
    // thread t holds the bins top, top - 1, ..., top - 7: the scan runs from the largest digit down
    const int top = nb - 1 - 8 * (int)tid;
    int sum = 0;
    for (int j = 0; j < 8; j++) if (top - j >= 0) sum += (int)hist[top - j];
    int total;
    const int excl = block_excl_scan(sum, ws, &total);
    if (pass == 0 && total <= k) { all = true; need = total; break; }
    if (excl < need && need <= excl + sum) {
      int acc = excl;
      for (int j = 0; j < 8 && top - j >= 0; j++) {
        const int c = (int)hist[top - j];
        if (acc + c >= need) { sel[0] = (uint32_t)(top - j); sel[1] = (uint32_t)(need - acc); break; }
        acc += c;
      }
    }
    block_barrier();
    prefix |= sel[0] << shift; mask |= (uint32_t)(nb - 1) << shift; need = (int)sel[1];
  }
  const int m = all ? need : k;                        // the length of the list
  const int above = all ? m : k - need;                // cells above t (every candidate, if all are taken): by cursor, in any order

  if (tid == 0) *cursor = 0u;
  block_barrier();
  int eq = 0;                                          // cells at t seen so far
  for (uint32_t base = 0; base < n; base += kTPB) {
    const uint32_t b = base + tid;
    uint32_t id = 0;
    const bool cand = b < n && signeigh_candidate<SELF>(row, a, b, minShared, table, minBits, &id);
    const uint64_t key = ((uint64_t)id << 32) | (uint64_t)(0xffffffffu - b);
    if (cand && (all || id > prefix)) {
      const uint32_t slot = atomicAdd(cursor, 1u);
      if (slot < (uint32_t)above) keys[slot] = key;
    }
    if (!all && eq < need) {                           // (the same in every thread)
      const int e = cand && id == prefix;
      int tot;
      const int rank = eq + block_excl_scan(e, ws, &tot);
      if (e && rank < need) keys[above + rank] = key;
      eq += tot;
    }
  }
  if (m > 0) block_sort(keys, m);                      // ascending; frames itself with barriers

  for (int i = tid; i < k; i += kTPB) {
    uint4 r;
    if (i < m) {
      const uint64_t key = keys[m - 1 - i];
      const uint32_t b = 0xffffffffu - (uint32_t)key, v = row[b];
      r.x = b; r.y = v >> 16; r.z = v & 0xffffu; r.w = (uint32_t)(key >> 32);
    } else { r.x = 0xffffffffu; r.y = 0u; r.z = 0u; r.w = 0u; }
    o[i] = r;
  }
  if (tid == 0) *cnt = m;
}

// One workgroup per row a = r0 + blockIdx.x of the strip; out and count are those of the whole row range, which begins at rowBegin.
static __global__ __launch_bounds__(kTPB) void k_signeigh_select(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t rowBegin, uint32_t n,
                                                                 int32_t minShared, const uint32_t *__restrict__ table, uint32_t minBits, int32_t k,
                                                                 uint4 *__restrict__ out, int32_t *__restrict__ count)
{
  __shared__ uint32_t hist[kSigNeighBins];
  __shared__ uint64_t keys[kSigNeighMaxK];
  __shared__ int ws[8];
  __shared__ uint32_t sel[2], cursor;
  const uint32_t a = r0 + blockIdx.x;
  signeigh_select_row<true>(hist, keys, ws, sel, &cursor, mat + (uint64_t)blockIdx.x * ld, a, n, minShared, table, minBits, k,
                            out + (uint64_t)(a - rowBegin) * (uint32_t)k, count + (a - rowBegin));
}

}  // namespace ani
