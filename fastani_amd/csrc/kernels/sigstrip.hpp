// sigstrip.hpp — the sketch pairs of a strip of genomes as edges of the single-linkage forest (ani_tree_single_sketch; no counterpart in
// the reference).  DESIGN.md section 2.16 states the algorithm; the host side is tree_single_sketch in engine_sig.hip.  The signatures are
// staged by k_sigpair_stage (sigdist.hpp); for the rows [r0, r1) of the pair matrix:
//
//   k_sigstrip_merge  the tiles of sigdist.hpp (sigpair_tile) counted from genome r0: cell (a, b > a) of an (r1 - r0) x ld strip,
//                     shared << 16 | size
//   k_sigstrip_count  per row a: every cell becomes bits(d) of its pair if the pair is an edge, else kSingleNone; the edges are counted
//   (device_scan of the row counts)
//   k_sigstrip_write  the edges of row a, b ascending, behind the row's offset: lo, hi, and bits(d) as a sort key with the position as
//                     its payload — what k_single_pairs yields for the pairs with rows
//
// A pair is an edge iff shared >= minShared, its d lies below d_missing (which an identity of 0 never does) and it has no rows: its key
// lo << b | hi is absent from the sorted distinct keys of the pairs with rows.  d comes from a table the host fills with its own double
// arithmetic, one entry per (shared, size) with 1 <= shared <= size; the device computes no logarithm.  One lane per pair, no atomics.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "sigdist.hpp"

namespace ani {

// entry of (shared, size), 1 <= shared <= size, in the table of distances
__host__ __device__ __forceinline__ uint32_t sigstrip_entry(uint32_t shared, uint32_t size) { return size * (size - 1) / 2 + (shared - 1); }

template <int T, int WORDS>
static __global__ __launch_bounds__(T * T >= kWave ? T * T : kWave) void k_sigstrip_merge(const uint32_t *__restrict__ sig, const int32_t *__restrict__ len,
    uint32_t n, uint32_t r0, uint32_t r1, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[2 * T];
  sigpair_tile<T>(tile, tileLen, sig, len, n, r0, r1, pitch, size, mat, ld);
}

// one workgroup per row a = r0 + blockIdx.x.  The keys of a's pairs with rows are one run of realKeys, found once per row.
static __global__ __launch_bounds__(kTPB) void k_sigstrip_count(uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t n, int32_t minShared,
                                                                const uint32_t *__restrict__ table, uint32_t dmBits, const uint64_t *__restrict__ realKeys,
                                                                uint32_t nKeys, int b, int32_t *__restrict__ rowCount)
{
  __shared__ int ws[8];
  __shared__ uint32_t run[2];
  const uint32_t a = r0 + blockIdx.x;
  uint32_t *row = mat + (uint64_t)blockIdx.x * ld;
  if (threadIdx.x == 0) {
    run[0] = sig_lower_bound(realKeys, nKeys, (uint64_t)a << b);
    run[1] = sig_lower_bound(realKeys, nKeys, ((uint64_t)a + 1) << b);
  }
  block_barrier();
  const uint64_t *keys = realKeys + run[0];
  const uint32_t nRun = run[1] - run[0];
  int c = 0;
  for (uint32_t hi = a + 1 + threadIdx.x; hi < n; hi += kTPB) {
    const uint32_t v = row[hi], shared = v >> 16, size = v & 0xffffu;
    uint32_t d = kSingleNone;
    if ((int32_t)shared >= minShared && shared <= size) {
      d = table[sigstrip_entry(shared, size)];
      if (d >= dmBits) d = kSingleNone;
      else if (nRun) {
        const uint64_t key = ((uint64_t)a << b) | hi;
        const uint32_t p = sig_lower_bound(keys, nRun, key);
        if (p < nRun && keys[p] == key) d = kSingleNone;
      }
    }
    row[hi] = d;
    c += d != kSingleNone;
  }
  int total;
  block_excl_scan(c, ws, &total);
  if (threadIdx.x == 0) rowCount[blockIdx.x] = total;
}

// one workgroup per row a = r0 + blockIdx.x: its edges from rowOff[blockIdx.x] on
static __global__ __launch_bounds__(kTPB) void k_sigstrip_write(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t n,
                                                                const uint32_t *__restrict__ rowOff, uint32_t *__restrict__ eLo, uint32_t *__restrict__ eHi,
                                                                uint64_t *__restrict__ dKey, uint32_t *__restrict__ idx)
{
  __shared__ int ws[8];
  const uint32_t a = r0 + blockIdx.x;
  const uint32_t *row = mat + (uint64_t)blockIdx.x * ld;
  uint32_t at = rowOff[blockIdx.x];
  for (uint32_t base = a + 1; base < n; base += kTPB) {
    const uint32_t hi = base + threadIdx.x;
    const uint32_t d = hi < n ? row[hi] : kSingleNone;
    const int keep = d != kSingleNone;
    int total;
    const int rank = block_excl_scan(keep, ws, &total);
    if (keep) { const uint32_t p = at + (uint32_t)rank; eLo[p] = a; eHi[p] = hi; dKey[p] = (uint64_t)d; idx[p] = p; }
    at += (uint32_t)total;
  }
}

}  // namespace ani
