// sigcluster.hpp — greedy representative clustering of the genomes under the whole-genome sketch estimate (ani_signature_cluster; no
// counterpart in the reference).  DESIGN.md section 2.20 states the algorithm; the host side is signature_cluster in engine_sig.hip.
// The signatures are staged by k_sigpair_stage (sigdist.hpp) and the cells come from k_sigscreen_merge (sigscreen.hpp), launched as it
// is: the strip's rows are its queries, and its references are either the signature rows of the representatives, kept contiguous in an
// array of their own, or the strip itself.  For the rows [r0, r1) of a strip:
//
//   k_sigcluster_best     one workgroup per row: the best edge of the row among the cells of a rows x representatives strip, folded into
//                         the genome's running best
//   k_sigcluster_resolve  one workgroup per strip: walks the rows in id order over the strip's own rows x rows block; a row without a
//                         best edge becomes a representative, and every row of the strip with an edge to it folds that edge
//   k_sigcluster_gather   one workgroup per new representative: its signature row and length appended to the representatives' array
//
// An edge is a cell with shared >= minShared whose identity bits, from the host's table (signeigh_candidate, signeigh.hpp), are at least
// minBits > 0.  The running best of genome g is the key identityBits << 32 | (0xffffffff - representative id), 0 while g has no edge to
// a representative, with the cell shared << 16 | size of that edge beside it: the largest key is the largest identity and, among equal
// identities, the smallest id (ani_abi.h, rule 3).  A maximum over a set, so no order of strips, tiles or lanes shows in it.  The slot
// of a genome has one writer in every kernel (lane 0 of the row's workgroup in k_sigcluster_best, lane g mod 256 in
// k_sigcluster_resolve), and kernels follow each other on one stream: no atomics.
//
// ani_signature_cluster_contain runs the same three kernels over other cells: shared << 16 | d of the containment
// walk in mode MAX (sigcontain.hpp), with the host's table of that estimate.  The kernels read a cell through the table only, and
// shared <= d <= size there as well, so nothing in them knows the estimate.  The strip's own block then comes from k_sigcontain_tri,
// which writes both cells of a pair and 0 on the diagonal; k_sigcluster_resolve skips the diagonal either way.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "signeigh.hpp"

namespace ani {

constexpr int kSigClusterMaxStrip = 4096;              // rows of a strip at the most: k_sigcluster_resolve keeps a word per row in LDS

__device__ __forceinline__ uint64_t sigcluster_key(uint32_t idBits, uint32_t id) { return ((uint64_t)idBits << 32) | (uint64_t)(0xffffffffu - id); }

// Row a = r0 + blockIdx.x of the strip against the nRef representatives whose ids are repId[0 .. nRef), ascending: cell b of the row is
// the pair (a, repId[b]).  The lanes reduce over the column, which orders like the id; lane 0 names the representative.
static __global__ __launch_bounds__(kTPB) void k_sigcluster_best(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t nRef,
                                                                 const uint32_t *__restrict__ repId, int32_t minShared, const uint32_t *__restrict__ table,
                                                                 uint32_t minBits, uint64_t *__restrict__ best, uint32_t *__restrict__ bestCell)
{
  __shared__ uint64_t top[kTPB / kWave];
  const uint32_t tid = threadIdx.x, a = r0 + blockIdx.x;
  const uint32_t *row = mat + (uint64_t)blockIdx.x * ld;
  uint64_t key = 0;
  for (uint32_t b = tid; b < nRef; b += kTPB) {
    uint32_t id;
    if (signeigh_candidate<false>(row, a, b, minShared, table, minBits, &id)) {
      const uint64_t k = sigcluster_key(id, b);
      key = k > key ? k : key;
    }
  }
  uint64_t o;
  o = lane_xor<32>(key); key = o > key ? o : key;
  o = lane_xor<16>(key); key = o > key ? o : key;
  o = lane_xor<8>(key); key = o > key ? o : key;
  o = lane_xor<4>(key); key = o > key ? o : key;
  o = lane_xor<2>(key); key = o > key ? o : key;
  o = lane_xor<1>(key); key = o > key ? o : key;
  if ((tid & (kWave - 1)) == 0) top[tid >> 6] = key;
  block_barrier();
  if (tid != 0) return;
  for (int w = 1; w < kTPB / kWave; w++) key = top[w] > key ? top[w] : key;
  if (key == 0) return;                                // no edge among these representatives
  const uint32_t b = 0xffffffffu - (uint32_t)key;
  const uint64_t k = sigcluster_key((uint32_t)(key >> 32), repId[b]);
  if (k > best[a]) { best[a] = k; bestCell[a] = row[b]; }
}

// The strip [r0, r0 + h), h <= kSigClusterMaxStrip, over its own h x h block (cell (i, j): the pair (r0 + i, r0 + j); the diagonal is
// the row against itself and is skipped).  covered[i]: row i has an edge to a representative.  Rows are taken in id order; covered[]
// changes only in the sweep of a new representative, which a barrier ends, so every lane reads the same covered[i] and members cost
// one LDS read.  A representative's sweep folds its edge into every row of the strip that has one: later rows become covered, earlier
// rows are members already (an earlier representative with an edge to this row would have covered it) and take the edge if it is their
// best.  Row j of the block belongs to lane j mod kTPB in every sweep.  memLen[g] = len[g] for a member and 0 for a representative: the
// lengths of the second sweep's queries, so that a representative costs no merge there.  The new representatives' ids go behind the
// nRep found before the strip, and the new count to *repCount.
static __global__ __launch_bounds__(kTPB) void k_sigcluster_resolve(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t r0, uint32_t h, uint32_t nRep,
                                                                    int32_t minShared, const uint32_t *__restrict__ table, uint32_t minBits,
                                                                    const int32_t *__restrict__ len, uint64_t *__restrict__ best, uint32_t *__restrict__ bestCell,
                                                                    int32_t *__restrict__ memLen, uint32_t *__restrict__ repId, uint32_t *__restrict__ repCount)
{
  __shared__ uint32_t covered[kSigClusterMaxStrip];
  const uint32_t tid = threadIdx.x;
  for (uint32_t j = tid; j < h; j += kTPB) covered[j] = best[r0 + j] != 0;
  block_barrier();
  for (uint32_t i = 0; i < h; i++) {
    if (covered[i]) continue;                          // (the same in every lane)
    if (tid == 0) repId[nRep] = r0 + i;
    nRep++;
    const uint32_t *row = mat + (uint64_t)i * ld;
    for (uint32_t j = tid; j < h; j += kTPB) {
      uint32_t id;
      if (j == i || !signeigh_candidate<false>(row, i, j, minShared, table, minBits, &id)) continue;
      const uint64_t k = sigcluster_key(id, r0 + i);
      if (k > best[r0 + j]) { best[r0 + j] = k; bestCell[r0 + j] = row[j]; }
      covered[j] = 1u;
    }
    block_barrier();
  }
  for (uint32_t j = tid; j < h; j += kTPB) memLen[r0 + j] = covered[j] ? len[r0 + j] : 0;
  if (tid == 0) *repCount = nRep;
}

// Representative number first + blockIdx.x: the staged row of genome repId[.] (whole quads, the tail zeroed) and its length.
static __global__ __launch_bounds__(kTPB) void k_sigcluster_gather(const uint32_t *__restrict__ sig, const int32_t *__restrict__ len,
                                                                   const uint32_t *__restrict__ repId, uint32_t first, int32_t pitch,
                                                                   uint32_t *__restrict__ repSig, int32_t *__restrict__ repLen)
{
  const uint32_t slot = first + blockIdx.x, g = repId[slot];
  const int32_t l = len[g];
  const uint4 *src = (const uint4 *)(sig + (uint64_t)g * (uint32_t)pitch);
  uint4 *dst = (uint4 *)(repSig + (uint64_t)slot * (uint32_t)pitch);
  for (uint32_t q = threadIdx.x; q < ((uint32_t)l + 3) / 4; q += kTPB) dst[q] = src[q];
  if (threadIdx.x == 0) repLen[slot] = l;
}

}  // namespace ani
