// siggraph.hpp — the pair graph of the genomes under the whole-genome sketch estimates, streamed (ani_signature_graph; no counterpart in
// the reference).  DESIGN.md section 2.21 states the algorithm; the host side is signature_graph in engine_sig.hip.  The signatures are
// staged by k_sigpair_stage (sigdist.hpp); for the rows [r0, r1) of the pair matrix:
//
//   (cells)           Mash: k_sigstrip_merge (sigstrip.hpp), the triangular tiles counted from genome r0.  Containment:
//                     k_sigcontain_merge (sigcontain.hpp) in mode ANI_CONTAIN_MAX with the strip as the queries and the genomes from r0
//                     on as the references.  Either way cell (a, b > a) of an (r1 - r0) x ld strip holds shared << 16 | size-or-d;
//                     cells with b <= a are never read.
//   k_siggraph_count  per row a, the cells (a, b > a) that are kept
//   (device_scan of the row counts)
//   k_siggraph_write  the kept cells of row a, b ascending, behind the row's offset: one ani_sigpair_t each, identity included
//
// A cell is kept iff shared >= minShared and its identity bits are at least those of minIdentity.  The bits come from a table the host
// fills with the double arithmetic of the chosen estimate, one entry per (shared, size-or-d) with 1 <= shared <= size-or-d
// (sigstrip_entry); the device computes no logarithm and no power.  Identities are non-negative floats, so their bit patterns order
// like their values.  One lane per cell, ranks from workgroup scans, no atomics: the order of the records is fixed by construction.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "sigdist.hpp"
#include "sigstrip.hpp"

namespace ani {

constexpr int kSigGraphRecordWords = 5;                // ani_sigpair_t: a, b, shared, size, identity
static_assert(sizeof(ani_sigpair_t) == 4 * kSigGraphRecordWords, "a record is five words");

// the identity bits of cell v, if the pair is kept (a cell with shared > size-or-d is no cell of the merge kernels: never kept)
__device__ __forceinline__ bool siggraph_keeps(uint32_t v, int32_t minShared, const uint32_t *__restrict__ table, uint32_t minBits, uint32_t *id)
{
  const uint32_t shared = v >> 16, size = v & 0xffffu;
  if ((int32_t)shared < minShared || shared > size) return false;
  *id = table[sigstrip_entry(shared, size)];
  return *id >= minBits;
}

// one workgroup per row a = r0 + blockIdx.x of the strip
static __global__ __launch_bounds__(kTPB) void k_siggraph_count(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t n, int32_t minShared,
                                                                const uint32_t *__restrict__ table, uint32_t minBits, int32_t *__restrict__ rowCount)
{
  __shared__ int ws[8];
  const uint32_t a = r0 + blockIdx.x;
  const uint32_t *row = mat + (uint64_t)blockIdx.x * ld;
  int c = 0;
  for (uint32_t b = a + 1 + threadIdx.x; b < n; b += kTPB) {
    uint32_t id;
    c += siggraph_keeps(row[b], minShared, table, minBits, &id);
  }
  int total;
  block_excl_scan(c, ws, &total);
  if (threadIdx.x == 0) rowCount[blockIdx.x] = total;
}

// one workgroup per row a = r0 + blockIdx.x: its kept pairs from record rowOff[blockIdx.x] of the strip on, in sweeps of kTPB columns
static __global__ __launch_bounds__(kTPB) void k_siggraph_write(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t n, int32_t minShared,
                                                                const uint32_t *__restrict__ table, uint32_t minBits, const uint32_t *__restrict__ rowOff,
                                                                uint32_t *__restrict__ out)
{
  __shared__ int ws[8];
  const uint32_t a = r0 + blockIdx.x;
  const uint32_t *row = mat + (uint64_t)blockIdx.x * ld;
  uint64_t at = rowOff[blockIdx.x];
  for (uint32_t base = a + 1; base < n; base += kTPB) {
    const uint32_t b = base + threadIdx.x;
    const uint32_t v = b < n ? row[b] : 0u;
    uint32_t id = 0;
    const int keep = b < n && siggraph_keeps(v, minShared, table, minBits, &id);
    int total;
    const int rank = block_excl_scan(keep, ws, &total);
    if (keep) {
      uint32_t *o = out + (at + (uint64_t)rank) * kSigGraphRecordWords;
      o[0] = a; o[1] = b; o[2] = v >> 16; o[3] = v & 0xffffu; o[4] = id;
    }
    at += (uint64_t)total;
  }
}

}  // namespace ani
