// sigscreen.hpp — the nearest references of every query genome under the whole-genome sketch estimate (ani_signature_screen; no
// counterpart in the reference).  DESIGN.md section 2.18 states the algorithm; the host side is signature_screen in engine_sig.hip.
// Both sets are staged by k_sigpair_stage (sigdist.hpp) into arrays of their own; for the queries [q0, q1) of a strip:
//
//   k_sigscreen_merge   one tile of TQ queries x TR references per workgroup, one merge per lane; cell (q - q0, r) of a (q1 - q0) x ld
//                       strip, shared << 16 | size.  The sets are distinct: every cell of a row is written.
//   k_sigscreen_select  one workgroup per query: the select of k_signeigh_select (signeigh.hpp) over a row without a self cell
//
// Two tile shapes.  The square one (TQ = TR = T, the T of the pair tiles at the same pitch) stages its TQ + TR rows in LDS and serves
// strips of at least T queries, where a staged reference row is used T times.  The thin one (TQ = 1, TR = 64) serves lower strips: a
// square tile would leave T - rows of its T lane rows idle there, and 1 + 64 rows of 1024 words do not fit the LDS of a tile.  It stages
// the query row alone, and every lane streams its reference row from global memory in 16-byte quads, one quad in registers at a time: a
// reference row has one reader in a tile of one query, so LDS would hold it for nothing.  A workgroup is one full wave of merges.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "sigdist.hpp"
#include "signeigh.hpp"

namespace ani {

constexpr int kSigScreenThinRefs = 64;                 // references per workgroup of the thin tile: one wave

// sig_merge_rows with row B in global memory, read a quad at a time (the row is staged: whole quads, the tail zeroed)
__device__ __forceinline__ uint32_t sig_merge_stream(const uint32_t *A, int32_t la, const uint4 *__restrict__ B4, int32_t lb, int32_t size)
{
  int32_t pa = 0, pb = 0, steps = 0, shared = 0;
  uint4 cur;
  cur.x = cur.y = cur.z = cur.w = 0u;
  if (lb > 0) cur = B4[0];
  while (steps < size && pa < la && pb < lb) {
    const int32_t c = pb & 3;
    const uint32_t x = A[pa], y = c == 0 ? cur.x : c == 1 ? cur.y : c == 2 ? cur.z : cur.w;
    const int32_t adv = y <= x;
    pa += x <= y; pb += adv; shared += x == y;
    steps++;
    if (adv && (pb & 3) == 0 && pb < lb) cur = B4[pb >> 2];
  }
  int32_t u = steps + (la - pa) + (lb - pb);
  if (u > size) u = size;
  return ((uint32_t)shared << 16) | (uint32_t)u;
}

// Workgroup (x, y): queries [q0 + TQ y, q0 + TQ y + TQ) against references [TR x, TR x + TR).  Lane (i, j) merges query row i with
// reference row j.  Queries at or beyond q1 and references at or beyond nRef have length 0 and no cell.
template <int TQ, int TR, int WORDS>
static __global__ __launch_bounds__(TQ * TR >= kWave ? TQ * TR : kWave) void k_sigscreen_merge(const uint32_t *__restrict__ refSig,
    const int32_t *__restrict__ refLen, uint32_t nRef, const uint32_t *__restrict__ qrySig, const int32_t *__restrict__ qryLen, uint32_t q0, uint32_t q1,
    int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  constexpr bool kStageRefs = TQ > 1;                  // the thin tile streams them
  constexpr int kRows = kStageRefs ? TQ + TR : TQ;
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[kRows];
  const uint32_t ty = blockIdx.y, tx = blockIdx.x;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t quads = (uint32_t)pitch / 4;
  uint4 *tile4 = (uint4 *)tile;
  for (uint32_t r = 0; r < (uint32_t)kRows; r++) {
    const bool isQry = r < (uint32_t)TQ;
    const uint64_t g = isQry ? (uint64_t)q0 + (uint64_t)ty * TQ + r : (uint64_t)tx * TR + (r - TQ);
    const int32_t l = g < (isQry ? q1 : nRef) ? (isQry ? qryLen : refLen)[g] : 0;
    if (tid == 0) tileLen[r] = l;
    const uint4 *src = (const uint4 *)((isQry ? qrySig : refSig) + g * (uint32_t)pitch);
    for (uint32_t q = tid; q < ((uint32_t)l + 3) / 4; q += nt) tile4[r * quads + q] = src[q];
  }
  block_barrier();
  if (tid >= (uint32_t)(TQ * TR)) return;
  const uint32_t i = tid / TR, j = tid % TR;
  const uint64_t a = (uint64_t)q0 + (uint64_t)ty * TQ + i, b = (uint64_t)tx * TR + j;
  if (a >= q1 || b >= nRef) return;
  uint32_t v;
  if (kStageRefs) v = sig_merge_rows(tile + i * (uint32_t)pitch, tileLen[i], tile + (TQ + j) * (uint32_t)pitch, tileLen[TQ + j], size);
  else v = sig_merge_stream(tile + i * (uint32_t)pitch, tileLen[i], (const uint4 *)(refSig + b * (uint32_t)pitch), refLen[b], size);
  mat[(a - q0) * ld + b] = v;
}

// One workgroup per query q = q0 + blockIdx.x of the strip: its row of nRef cells -> its k records and its count.
static __global__ __launch_bounds__(kTPB) void k_sigscreen_select(const uint32_t *__restrict__ mat, uint64_t ld, uint32_t q0, uint32_t nRef, int32_t minShared,
                                                                  const uint32_t *__restrict__ table, uint32_t minBits, int32_t k, uint4 *__restrict__ out,
                                                                  int32_t *__restrict__ count)
{
  __shared__ uint32_t hist[kSigNeighBins];
  __shared__ uint64_t keys[kSigNeighMaxK];
  __shared__ int ws[8];
  __shared__ uint32_t sel[2], cursor;
  const uint32_t q = q0 + blockIdx.x;
  signeigh_select_row<false>(hist, keys, ws, sel, &cursor, mat + (uint64_t)blockIdx.x * ld, q, nRef, minShared, table, minBits, k,
                             out + (uint64_t)q * (uint32_t)k, count + q);
}

}  // namespace ani
