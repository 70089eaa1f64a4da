// sigdist.hpp — whole-genome sketch ANI: bottom-s signatures of the reference genomes out of their minimizer records, and the
// all-pairs comparison of signatures (ani_sketch_signatures, ani_signature_pairs; no counterpart in the reference, which knows no
// genome-level sketch).  DESIGN.md section 2.14 states the algorithm; the host side is in engine_sig.hip.
//
//   signatures, per index chunk (records = the chunk's index arrays, or the 12-byte records a streamed set keeps):
//   k_sig_count     per block of kSigBlock records, the records whose hash is at or below their genome's threshold
//   (device_scan of the block counts)
//   k_sig_keys      the survivors as keys genome << 32 | hash, behind their block's offset
//   (the radix sort of the keys)
//   k_sig_emit      per genome, the first `size` distinct hashes of its run of keys -> its signature row and length
//
//   pairs:
//   k_sigpair_stage the uploaded rows to a pitch of whole 16-byte quads; a row that does not ascend strictly sets a flag
//   k_sigpair_merge one tile of T x T pairs per workgroup: the 2 T rows in LDS, one two-pointer merge per lane -> shared << 16 | size
//   k_sigpair_count per row a, the pairs (a, b > a) with shared >= minShared
//   (device_scan of the row counts)
//   k_sigpair_write the kept pairs of row a, b ascending, behind the row's offset
#pragma once
#include "../../../include/ani_abi.h"
#include "common.hpp"

namespace ani {

constexpr int kSigBlock = 2048;                        // records per workgroup of k_sig_count / k_sig_keys
constexpr int kSigMaxSize = 4096;                      // largest signature (ani_abi.h)
constexpr int kSigTileWords = 32768;                   // LDS of the large merge tiles: 128 KiB of the CU's 160

// Where a chunk's records are: the index arrays (stride 1, chunk-local seqIds) or 12-byte records (stride 3, seqIds of the set).
struct SigSource { const uint32_t *hash; const int32_t *seq; uint32_t stride; int32_t seqBase; uint64_t n; };

// threshold of a genome: a record takes part iff (int64) hash <= thr; -1 = the genome is left out of this round
__device__ __forceinline__ bool sig_takes(const SigSource &s, uint64_t i, const int32_t *__restrict__ contigGenome, const int64_t *__restrict__ thr,
                                          uint64_t *key)
{
  const uint32_t h = s.hash[i * s.stride];
  const int32_t g = contigGenome[s.seq[i * s.stride] - s.seqBase];
  *key = ((uint64_t)(uint32_t)g << 32) | h;
  return (int64_t)h <= thr[g];
}

static __global__ __launch_bounds__(kTPB) void k_sig_count(SigSource s, const int32_t *__restrict__ contigGenome, const int64_t *__restrict__ thr,
                                                           int32_t *__restrict__ blockCount)
{
  __shared__ int ws[8];
  const uint64_t base = (uint64_t)blockIdx.x * kSigBlock;
  int c = 0;
  for (int e = threadIdx.x; e < kSigBlock; e += kTPB) {
    uint64_t key;
    if (base + e < s.n && sig_takes(s, base + e, contigGenome, thr, &key)) c++;
  }
  int total;
  block_excl_scan(c, ws, &total);
  if (threadIdx.x == 0) blockCount[blockIdx.x] = total;
}

// (the order of the keys inside a block is whatever the LDS cursor gives: the sort that follows makes the result independent of it)
static __global__ __launch_bounds__(kTPB) void k_sig_keys(SigSource s, const int32_t *__restrict__ contigGenome, const int64_t *__restrict__ thr,
                                                          const uint32_t *__restrict__ blockOff, uint64_t *__restrict__ keys)
{
  __shared__ uint32_t cursor;
  if (threadIdx.x == 0) cursor = 0;
  block_barrier();
  const uint64_t base = (uint64_t)blockIdx.x * kSigBlock;
  const uint32_t off = blockOff[blockIdx.x];
  for (int e = threadIdx.x; e < kSigBlock; e += kTPB) {
    uint64_t key;
    if (base + e < s.n && sig_takes(s, base + e, contigGenome, thr, &key)) keys[off + atomicAdd(&cursor, 1u)] = key;
  }
}

// first index of the sorted keys whose key is >= x
__device__ __forceinline__ uint32_t sig_lower_bound(const uint64_t *__restrict__ keys, uint32_t n, uint64_t x)
{
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (keys[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// One workgroup per genome of the chunk (a genome left out of the round keeps what it has): the distinct hashes of its run of the
// sorted keys are numbered by a scan, the first `size` go to its row, the rest of the row is zeroed.
static __global__ __launch_bounds__(kTPB) void k_sig_emit(const uint64_t *__restrict__ keys, uint32_t nKeys, const int64_t *__restrict__ thr, int32_t size,
                                                          uint32_t *__restrict__ sig, int32_t *__restrict__ len)
{
  __shared__ int ws[8];
  const uint32_t g = blockIdx.x;
  if (thr[g] < 0) return;
  const uint32_t lo = sig_lower_bound(keys, nKeys, (uint64_t)g << 32), hi = sig_lower_bound(keys, nKeys, ((uint64_t)g + 1) << 32);
  uint32_t *row = sig + (uint64_t)g * (uint32_t)size;
  int have = 0;
  for (uint32_t base = lo; base < hi && have < size; base += kTPB) {
    const uint32_t i = base + threadIdx.x;
    const int first = i < hi && (i == lo || keys[i] != keys[i - 1]);
    int total;
    const int rank = have + block_excl_scan(first, ws, &total);
    if (first && rank < size) row[rank] = (uint32_t)keys[i];
    have += total;
  }
  if (have > size) have = size;
  for (int r = have + (int)threadIdx.x; r < size; r += kTPB) row[r] = 0u;
  if (threadIdx.x == 0) len[g] = have;
}

// ---- pairs ----

// rows of `size` values -> rows of `pitch` (a multiple of 4: 16-byte loads of whole rows), the tail zeroed; bad[0] |= 1 where a row
// does not ascend strictly inside its length.  One workgroup per genome.
static __global__ __launch_bounds__(kTPB) void k_sigpair_stage(const uint32_t *__restrict__ in, const int32_t *__restrict__ len, int32_t size, int32_t pitch,
                                                               uint32_t *__restrict__ out, uint32_t *__restrict__ bad)
{
  const uint32_t g = blockIdx.x;
  const uint32_t *src = in + (uint64_t)g * (uint32_t)size;
  uint32_t *dst = out + (uint64_t)g * (uint32_t)pitch;
  const int l = len[g];
  bool wrong = false;
  for (int r = threadIdx.x; r < pitch; r += kTPB) {
    const uint32_t v = r < l ? src[r] : 0u;
    if (r > 0 && r < l && src[r - 1] >= v) wrong = true;
    dst[r] = v;
  }
  if (wrong) atomicOr(bad, 1u);
}

// The hot path.  Workgroup (x, y) with x >= y compares genomes [T y, T y + T) with genomes [T x, T x + T): their rows go to LDS with
// 16-byte loads (a diagonal tile holds its rows once), then lane (i, j) merges row i with row j from there.  One step takes the next
// element of the ascending distinct union U: the smaller head advances, both on a tie, which is a shared value.  The walk ends after
// `size` elements of U or when a row is used up; from there U only has the other row's tail, which shares nothing:
//   size(a, b) = min(size, steps + what is left of either row),   shared(a, b) = ties among the steps.
// Integers only and one lane per pair: no atomics, no dependence on any order.  T and the LDS words are chosen by the host from the
// row pitch (sigpair_launch in engine_sig.hip); pairs with b <= a, and genomes beyond n, are skipped.
// sigpair_tile is the tile itself, shared with the strip kernel (sigstrip.hpp): tile coordinates count from genome `base`, rows end at
// rowEnd, and the cell of (a, b) is mat[(a - base) * ld + b].  The whole matrix is base = 0, rowEnd = n.
// the merge of one pair, rows A and B of lengths la and lb (in LDS): shared << 16 | size
__device__ __forceinline__ uint32_t sig_merge_rows(const uint32_t *A, int32_t la, const uint32_t *B, int32_t lb, int32_t size)
{
  int32_t pa = 0, pb = 0, steps = 0, shared = 0;
  while (steps < size && pa < la && pb < lb) {
    const uint32_t x = A[pa], y = B[pb];
    pa += x <= y; pb += y <= x; shared += x == y;
    steps++;
  }
  int32_t u = steps + (la - pa) + (lb - pb);
  if (u > size) u = size;
  return ((uint32_t)shared << 16) | (uint32_t)u;
}

template <int T>
__device__ __forceinline__ void sigpair_tile(uint32_t *tile, int32_t *tileLen, const uint32_t *__restrict__ sig, const int32_t *__restrict__ len, uint32_t n,
    uint32_t base, uint32_t rowEnd, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  const uint32_t ty = blockIdx.y, tx = blockIdx.x;
  if (tx < ty) return;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const bool diag = tx == ty;
  const uint32_t rows = diag ? T : 2 * T, quads = (uint32_t)pitch / 4;
  uint4 *tile4 = (uint4 *)tile;
  for (uint32_t r = 0; r < rows; r++) {
    const uint64_t g = (uint64_t)base + (r < (uint32_t)T ? (uint64_t)ty * T : (uint64_t)tx * T - T) + r;
    const int32_t l = g < n ? len[g] : 0;
    if (tid == 0) tileLen[r] = l;
    const uint4 *src = (const uint4 *)(sig + g * (uint32_t)pitch);
    for (uint32_t q = tid; q < ((uint32_t)l + 3) / 4; q += nt) tile4[r * quads + q] = src[q];
  }
  block_barrier();
  if (tid >= (uint32_t)(T * T)) return;
  const uint32_t i = tid / T, j = tid % T;
  const uint64_t a = (uint64_t)base + (uint64_t)ty * T + i, b = (uint64_t)base + (uint64_t)tx * T + j;
  if (a >= b || b >= n || a >= rowEnd) return;
  const uint32_t rb = diag ? j : T + j;
  const uint32_t *A = tile + i * (uint32_t)pitch, *B = tile + rb * (uint32_t)pitch;
  mat[(a - base) * ld + b] = sig_merge_rows(A, tileLen[i], B, tileLen[rb], size);
}

template <int T, int WORDS>
static __global__ __launch_bounds__(T * T >= kWave ? T * T : kWave) void k_sigpair_merge(const uint32_t *__restrict__ sig, const int32_t *__restrict__ len,
    int32_t n, int32_t pitch, int32_t size, uint32_t *__restrict__ mat, uint64_t ld)
{
  __shared__ uint32_t tile[WORDS];
  __shared__ int32_t tileLen[2 * T];
  sigpair_tile<T>(tile, tileLen, sig, len, (uint32_t)n, 0u, (uint32_t)n, pitch, size, mat, ld);
}

// one workgroup per row a
static __global__ __launch_bounds__(kTPB) void k_sigpair_count(const uint32_t *__restrict__ mat, uint64_t ld, int32_t n, int32_t minShared,
                                                               int32_t *__restrict__ rowCount)
{
  __shared__ int ws[8];
  const uint32_t a = blockIdx.x;
  const uint32_t *row = mat + (uint64_t)a * ld;
  int c = 0;
  for (uint32_t b = a + 1 + threadIdx.x; b < (uint32_t)n; b += kTPB) c += (int32_t)(row[b] >> 16) >= minShared;
  int total;
  block_excl_scan(c, ws, &total);
  if (threadIdx.x == 0) rowCount[a] = total;
}

// one workgroup per row a: its kept pairs {a, b, shared, size}, b ascending, from rowOff[a] on
static __global__ __launch_bounds__(kTPB) void k_sigpair_write(const uint32_t *__restrict__ mat, uint64_t ld, int32_t n, int32_t minShared,
                                                               const uint32_t *__restrict__ rowOff, uint4 *__restrict__ out)
{
  __shared__ int ws[8];
  const uint32_t a = blockIdx.x;
  const uint32_t *row = mat + (uint64_t)a * ld;
  uint64_t at = rowOff[a];
  for (uint32_t base = a + 1; base < (uint32_t)n; base += kTPB) {
    const uint32_t b = base + threadIdx.x;
    const uint32_t v = b < (uint32_t)n ? row[b] : 0u;
    const int keep = b < (uint32_t)n && (int32_t)(v >> 16) >= minShared;
    int total;
    const int rank = block_excl_scan(keep, ws, &total);
    if (keep) { uint4 o; o.x = a; o.y = b; o.z = v >> 16; o.w = v & 0xffffu; out[at + (uint64_t)rank] = o; }
    at += (uint64_t)total;
  }
}

}  // namespace ani
