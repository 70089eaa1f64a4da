// boot.hpp — the bootstrap replicate sums of the ANI values as records (ani_sketch_boot_begin / _take): what
// k_ci_records (ci.hpp) draws and reduces to two order statistics, kept — the input of the trees' support values (ani_tree_support).
//
// The values, the gate and the draws are the intervals' (ani_abi.h; ci.hpp): for every pair that passes this mode's own gate the
// non-empty cells of the genome's bins in bin order are the sample, F[i] = fix(cell i), and replicate r adds the F at `count` positions
// of the stated counter-based hash up to S[r].  The gate and the list are the intervals' two kernels, k_ci_flags and k_ci_list, under
// this mode's CiArgs (as synteny reuses the hits'); the gather and the draw are ci_gather and ci_replicate.
//   k_boot_records  one workgroup of 256 per listed pair: ci_gather leaves F in LDS — or, for a pair with more cells than the cap, in the
//                   pair's run of the device pool — with minimum, maximum and sum.  A pair whose minimum equals its maximum has S[r] = sum.
//                   Else thread t takes the replicates t, t + 256, ...: one fmix32, one multiply-high and one read of F per draw, the
//                   64-bit sum in registers.  S[r] goes to sums[pair * B + r]: a wave stores 64 consecutive uint64, and a pair's run
//                   follows its predecessor's.  Thread 0 writes the 24-byte record.  No floating point after fix, no scratch.
// LDS: 2560 cells (10 KiB) and the gather's 112 bytes; no sums are kept on chip, they are not ranked here.
#pragma once
#include "ci.hpp"

namespace ani {

// one record as the host receives it (ani_boot_t of ani_abi.h; qry = the query's index in the sub-batch)
struct BootRec { int32_t ref, qry; uint32_t count, replicates; unsigned long long sum; };
static_assert(sizeof(BootRec) == 24, "record layout");

// pairs [first, first + n) of the list -> rec[0 .. n) and sums[0 .. n * replicates); a pair above the cap keeps its cells at
// pool[poolOff[pair] - poolBase ..)
static __global__ __launch_bounds__(kTPB) void k_boot_records(CiArgs a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ poolOff,
                                                       uint32_t first, uint32_t n, uint32_t poolBase, uint32_t *pool, BootRec *__restrict__ rec,
                                                       unsigned long long *__restrict__ sums)
{
  __shared__ uint32_t sF[kCiLdsCells];
  __shared__ unsigned long long sSum[kTPB / kWave];
  __shared__ uint32_t sCnt[2][kTPB / kWave], sMin[kTPB / kWave], sMax[kTPB / kWave];
  const uint32_t r = blockIdx.x;
  if (r >= n) return;                                   // block-uniform
  const uint32_t t = threadIdx.x;
  const uint32_t p = list[first + r];
  const int qi = (int)(p / (uint32_t)a.nRefGenomes), g = (int)(p % (uint32_t)a.nRefGenomes);
  const uint32_t count = a.pairCount[(size_t)qi * (size_t)a.outStride + (size_t)a.outCol0 + (size_t)g];   // = the non-empty cells of g
  const bool big = count > a.ldsCells;                  // block-uniform
  uint32_t *gF = pool + (big ? poolOff[first + r] - poolBase : 0u);

  uint32_t mn, mx;
  unsigned long long sum;
  ci_gather(a, qi, g, count, big, gF, sF, sCnt, sMin, sMax, sSum, mn, mx, sum);

  const uint32_t B = a.replicates;
  unsigned long long *out = sums + (size_t)r * B;
  const bool one = mn == mx;                            // block-uniform; one distinct value: every replicate is the sum
  for (uint32_t q = t; q < B; q += kTPB) {
    unsigned long long s = sum;
    if (!one) {
      const uint32_t k = ci_fmix32(a.seed + 0x9e3779b9u * (q + 1u));
      s = big ? ci_replicate(gF, count, k) : ci_replicate(sF, count, k);
    }
    out[q] = s;
  }
  if (t == 0) {
    BootRec o;
    o.ref = a.genomeBase + g; o.qry = qi; o.count = count; o.replicates = B; o.sum = sum;
    rec[r] = o;
  }
}

}  // namespace ani
