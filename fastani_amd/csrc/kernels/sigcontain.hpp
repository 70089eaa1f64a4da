// sigcontain.hpp — the nearest references of every query genome under the containment estimate (ani_signature_screen_contain; no
// counterpart in the reference).  DESIGN.md section 2.19 states the algorithm; the host side is signature_screen_contain in
// engine_sig.hip.  Staging, strips, tile shapes and the select are those of sigscreen.hpp; what differs is the walk of a pair and what
// its cell holds:
//
//   k_sigcontain_merge  one tile of TQ queries x TR references per workgroup, one walk per lane; cell (q - q0, r) of a (q1 - q0) x ld
//                       strip, shared << 16 | d, d the denominator of the mode (ani_abi.h rules 2 - 4)
//   (k_sigscreen_select of sigscreen.hpp, unchanged: shared <= d <= size, so the cell and the triangular table fit as they are)
//   k_sigcontain_tri    the rows x rows block of a strip against itself in mode MAX, from its upper triangle alone: one walk per pair,
//                       both cells written (ani_signature_cluster_contain)
//
// The walk.  Q and R ascend strictly; one step looks at the heads x = Q[pa], y = R[pb], the smaller advances, both on a tie, which is a
// shared value.  Unlike sig_merge_rows there is no cap at `size` union elements: the walk ends when either row ends, after at most
// lq + lr - shared steps, and every value of both lists that can be shared has then been met, so `shared` is over the whole of both.
// The pointer identity.  A value of Q is passed only in a step with x <= y, and y <= last(R) always: every passed value of Q is
// <= last(R).  If R ends first (pb = lr), the step that passed last(R) had y = last(R) <= x: on a tie x is passed with it and the next
// value of Q is larger, otherwise x itself is larger; either way Q[pa] > last(R) from there on, since Q ascends.  So pa is exactly the
// number of values of Q that are <= last(R).  If Q ends first, pa = lq, and all of Q is <= the head of R it met last, <= last(R).  In
// both cases
//   inQ = (lr == size) ? pa : lq        and by the same argument with the roles swapped        inR = (lq == size) ? pb : lr.
// An empty row ends the walk before its first step: pa = pb = 0, shared = 0, no candidate whatever d is.
//
// The mode is a kernel argument, not a template parameter: it is read once after the walk, in three scalar compares and two selects, and
// costs no VGPR (DESIGN.md 2.19 has the counts); as a template parameter it would triple the six instances for nothing inside the loop.
//
// LDS of the square tile.  ds_read_b32 has 32 banks and rows start on whole quads, so the rows of a tile start on at most 8 distinct
// banks, and on fewer when pitch / 4 is even (1000 words: 4; 1024 words: 1).  This walk is up to twice as long as the Mash merge, so the
// tile keeps its rows at a pitch of their own in LDS: pitch + 4 words where pitch / 4 is even, which makes pitch / 4 odd and the row
// starts cycle through all 8.  WORDS has room for that: 4 words more for each of the at most 32 rows.
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"
#include "sigdist.hpp"
#include "sigscreen.hpp"

namespace ani {

constexpr int kSigContainPad = 128;                    // words beyond the rows of a square tile: 4 for each of up to 32 rows

// the cell of a pair from the end of its walk: Q of length lq walked to pa, R of length lr walked to pb
__device__ __forceinline__ uint32_t sig_contain_cell(int32_t lq, int32_t lr, int32_t pa, int32_t pb, int32_t shared, int32_t size, int32_t mode)
{
  const int32_t inQ = lr == size ? pa : lq, inR = lq == size ? pb : lr;
  const int32_t d = mode == ANI_CONTAIN_QUERY ? inQ : mode == ANI_CONTAIN_REF ? inR : (inQ < inR ? inQ : inR);
  return ((uint32_t)shared << 16) | (uint32_t)d;
}

// query row A and reference row B, both in LDS
__device__ __forceinline__ uint32_t sig_contain_rows(const uint32_t *A, int32_t la, const uint32_t *B, int32_t lb, int32_t size, int32_t mode)
{
  int32_t pa = 0, pb = 0, shared = 0;
  while (pa < la && pb < lb) {
    const uint32_t x = A[pa], y = B[pb];
    pa += x <= y; pb += y <= x; shared += x == y;
  }
  return sig_contain_cell(la, lb, pa, pb, shared, size, mode);
}

// the same with row B in global memory, read a quad at a time (the row is staged: whole quads, the tail zeroed).  Only B[pb] with
// pb < lb is ever looked at, so a zero of the tail is never taken for a value and a first value of 0 is one; lb = 0 loads nothing, and a
// row that ends on a quad border loads no quad beyond it.
__device__ __forceinline__ uint32_t sig_contain_stream(const uint32_t *A, int32_t la, const uint4 *__restrict__ B4, int32_t lb, int32_t size, int32_t mode)
{
  int32_t pa = 0, pb = 0, shared = 0;
  uint4 cur;
  cur.x = cur.y = cur.z = cur.w = 0u;
  if (lb > 0) cur = B4[0];
  while (pa < la && pb < lb) {
    const int32_t c = pb & 3;
    const uint32_t x = A[pa], y = c == 0 ? cur.x : c == 1 ? cur.y : c == 2 ? cur.z : cur.w;
    const int32_t adv = y <= x;
    pa += x <= y; pb += adv; shared += x == y;
    if (adv && (pb & 3) == 0 && pb < lb) cur = B4[pb >> 2];
  }
  return sig_contain_cell(la, lb, pa, pb, shared, size, mode);
}

// Workgroup (x, y): queries [q0 + TQ y, q0 + TQ y + TQ) against references [TR x, TR x + TR).  Lane (i, j) walks query row i and
// reference row j.  Queries at or beyond q1 and references at or beyond nRef have length 0 and no cell.  WORDS >= the rows in LDS at
// their LDS pitch: (TQ + TR) (pitch + 4) for the square tile, pitch for the thin one.
template <int TQ, int TR, int WORDS>
static __global__ __launch_bounds__(TQ * TR >= kWave ? TQ * TR : kWave) void k_sigcontain_merge(const uint32_t *__restrict__ refSig,
    const int32_t *__restrict__ refLen, uint32_t nRef, const uint32_t *__restrict__ qrySig, const int32_t *__restrict__ qryLen, uint32_t q0, uint32_t q1,
    int32_t pitch, int32_t size, int32_t mode, uint32_t *__restrict__ mat, uint64_t ld)
{
  constexpr bool kStageRefs = TQ > 1;                  // the thin tile streams them
  constexpr int kRows = kStageRefs ? TQ + TR : TQ;
  static_assert(!kStageRefs || kRows * 4 <= kSigContainPad, "the pad holds 4 words per row");
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[kRows];
  const uint32_t ty = blockIdx.y, tx = blockIdx.x;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t ldsPitch = (uint32_t)pitch + (kStageRefs && ((pitch >> 2) & 1) == 0 ? 4u : 0u);
  const uint32_t quads = ldsPitch / 4;
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
  if (kStageRefs) v = sig_contain_rows(tile + i * ldsPitch, tileLen[i], tile + (TQ + j) * ldsPitch, tileLen[TQ + j], size, mode);
  else v = sig_contain_stream(tile + i * ldsPitch, tileLen[i], (const uint4 *)(refSig + b * (uint32_t)pitch), refLen[b], size, mode);
  mat[(a - q0) * ld + b] = v;
}

// The h x h block of the rows [0, h) of sig against themselves in mode ANI_CONTAIN_MAX, where cell (i, j) equals cell (j, i): `shared` is
// symmetric, and d = min(inQ, inR) with the roles swapped.  Only the tiles on or above the diagonal are launched, as a linear grid of
// n (n + 1) / 2 workgroups, n = ceil(h / T): workgroup t is tile (ty <= tx) with t = tx (tx + 1) / 2 + ty, so tx is the largest integer
// with tx (tx + 1) / 2 <= t (a float square root, then exact integer steps: 8 t + 1 < 2^24 for every h the callers have).  A tile right
// of the diagonal stages 2 T rows and lane (i, j) walks its pair once; a tile on the diagonal stages its T rows once, and only the
// lanes with j > i walk.  Either way the lane writes cell (a, b) and its mirror (b, a), the latter strided by ld.  The diagonal cells
// are written as 0: k_sigcluster_resolve skips them, and no cell of the block is left as it was.  Rows at or beyond h have length 0 and
// no cell.  WORDS >= 2 T (pitch + 4), as for the square tile of k_sigcontain_merge, whose LDS pitch this keeps.
template <int T, int WORDS>
static __global__ __launch_bounds__(T * T >= kWave ? T * T : kWave) void k_sigcontain_tri(const uint32_t *__restrict__ sig, const int32_t *__restrict__ len,
    uint32_t h, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  static_assert(2 * T * 4 <= kSigContainPad, "the pad holds 4 words per row");
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[2 * T];
  const uint32_t t = blockIdx.x;
  uint32_t tx = (uint32_t)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (tx * (tx + 1) / 2 > t) tx--;
  while ((tx + 1) * (tx + 2) / 2 <= t) tx++;
  const uint32_t ty = t - tx * (tx + 1) / 2;
  const bool diag = ty == tx;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t ldsPitch = (uint32_t)pitch + (((pitch >> 2) & 1) == 0 ? 4u : 0u);
  const uint32_t quads = ldsPitch / 4;
  const uint32_t rows = diag ? (uint32_t)T : 2u * T, colRow0 = diag ? 0u : (uint32_t)T;       // a diagonal tile's columns are its rows
  uint4 *tile4 = (uint4 *)tile;
  for (uint32_t r = 0; r < rows; r++) {
    const uint32_t g = r < (uint32_t)T ? ty * T + r : tx * T + (r - T);
    const int32_t l = g < h ? len[g] : 0;
    if (tid == 0) tileLen[r] = l;
    const uint4 *src = (const uint4 *)(sig + (uint64_t)g * (uint32_t)pitch);
    for (uint32_t q = tid; q < ((uint32_t)l + 3) / 4; q += nt) tile4[r * quads + q] = src[q];
  }
  block_barrier();
  if (tid >= (uint32_t)(T * T)) return;
  const uint32_t i = tid / T, j = tid % T;
  const uint64_t a = (uint64_t)ty * T + i, b = (uint64_t)tx * T + j;
  if (a >= h || b >= h || b < a) return;               // (b < a: left of the diagonal in a diagonal tile, the mirror of a lane that walks)
  if (a == b) { mat[a * ld + a] = 0u; return; }
  const uint32_t v = sig_contain_rows(tile + i * ldsPitch, tileLen[i], tile + (colRow0 + j) * ldsPitch, tileLen[colRow0 + j], size, ANI_CONTAIN_MAX);
  mat[a * ld + b] = v;
  mat[b * ld + a] = v;
}

}  // namespace ani
