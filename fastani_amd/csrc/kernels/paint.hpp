// paint.hpp — per-fragment best reference over the whole reference set (ani_sketch_paint_begin / _take; no counterpart in the reference,
// whose outputs are all per pair of genomes).  DESIGN.md section 2.27.
//
// reduce_stage has the candidates of one (sub-batch, index chunk) in the context's buffers, ordered so that the mappings of one
// (fragment, reference genome) are adjacent (reduce.hpp).  For every fragment with at least one 1-way winner one partial record is made:
// the genome with the best winner — larger identity bits first, then the smaller genome id —, that winner's contig and position, the
// second genome under the same order with its winner's bits, and the number of genomes that have a winner.  The host joins the partial
// records a fragment gets from the chunks of a set (ani_paint_merge).  Everything is integer or bit pattern; the only read-modify-write
// operations are integer maxima and integer sums, so nothing depends on an order.
//   k_paint_best     one lane per candidate; a (fragment, genome) group head resolves its group exactly as k_oneway_bins does and does a
//                    64-bit atomicMax(best[f], bits << 32 | ~genome) — genome = the set-global id, complemented so that the smaller id
//                    wins at equal bits — and atomicAdd(genomes[f], 1).
//   k_paint_second   a launch of its own, the same walk: the head whose key is best[f] stores the index of its winning candidate in
//                    win[f] (one writer: a genome has one group per fragment); every other head does atomicMax(second[f], key).
//   k_paint_flags    genomes[f] != 0 -> flag; device_scan gives the record slots, in fragment order = (query, querySeqId) order.
//   k_paint_records  one lane per fragment: the records whose slot falls into [recBase, recBase + n) are written to out[slot - recBase].
// State: 24 bytes per fragment of the sub-batch (best, second: 8 each; genomes, win: 4 each), held only while the mode is on.  No LDS, no
// scratch.
#pragma once
#include "common.hpp"
#include "reduce.hpp"

namespace ani {

struct PaintArgs {
  OneWayArgs w;                                // the candidates, as k_oneway_bins got them (the bin table is not touched)
  const int32_t *fragQSeq;                     // fragment -> querySeqId
  int32_t nFrag;
  int32_t genomeBase, seqBase;                 // set-global ids of the chunk's first genome and contig
  unsigned long long *best, *second;           // [nFrag] bits << 32 | ~(set-global genome); 0 = none
  uint32_t *genomes, *win;                     // [nFrag] genomes with a winner; the best genome's winning candidate
};

// one partial record as the host receives it (ani_paint_t of ani_abi.h, the identities as bits; qry = the query's index in the sub-batch)
struct PaintRec { int32_t qry, qSeq, ref, refSeq, refStart; uint32_t idBits; int32_t second; uint32_t secondBits, genomes, reserved; };
static_assert(sizeof(PaintRec) == 40, "record layout");

// candidate c as a group head: the group's 1-way winner (k_oneway_bins' walk and order) -> the fragment, the winning candidate and the
// key bits << 32 | ~genome; false: no head, or no mapping with identity bits
__device__ __forceinline__ bool paint_head(const PaintArgs &p, int c, int *frag, int *win, unsigned long long *key)
{
  const OneWayArgs &a = p.w;
  const int f = a.candFrag[c];
  const int g = a.contigGenome[a.candSeq[c]];
  if (c > 0 && a.candFrag[c - 1] == f && a.contigGenome[a.candSeq[c - 1]] == g) return false;
  uint32_t bBits = 0; int32_t bSeq = -1, bPos = -1; int bAt = -1;
  for (int x = c; x < a.nCand && a.candFrag[x] == f && a.contigGenome[a.candSeq[x]] == g; x++) {
    const uint32_t bits = a.idBits[x];
    if (!bits) continue;
    const int32_t sq = a.candSeq[x], ps = a.refStart[x];
    if (bits > bBits || (bits == bBits && (sq > bSeq || (sq == bSeq && ps > bPos)))) { bBits = bits; bSeq = sq; bPos = ps; bAt = x; }
  }
  if (!bBits || (unsigned)f >= (unsigned)p.nFrag) return false;
  *frag = f; *win = bAt;
  *key = ((unsigned long long)bBits << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(p.genomeBase + g));
  return true;
}

static __global__ __launch_bounds__(kTPB) void k_paint_best(PaintArgs p)
{
  const int c = blockIdx.x * kTPB + threadIdx.x;
  if (c >= p.w.nCand) return;
  int f, win; unsigned long long key;
  if (paint_head(p, c, &f, &win, &key)) { atomicMax(&p.best[f], key); atomicAdd(&p.genomes[f], 1u); }
}

static __global__ __launch_bounds__(kTPB) void k_paint_second(PaintArgs p)
{
  const int c = blockIdx.x * kTPB + threadIdx.x;
  if (c >= p.w.nCand) return;
  int f, win; unsigned long long key;
  if (!paint_head(p, c, &f, &win, &key)) return;
  if (p.best[f] == key) p.win[f] = (uint32_t)win;
  else atomicMax(&p.second[f], key);
}

static __global__ __launch_bounds__(kTPB) void k_paint_flags(PaintArgs p, int32_t *__restrict__ flags)
{
  const int f = blockIdx.x * kTPB + threadIdx.x;
  if (f < p.nFrag) flags[f] = p.genomes[f] != 0 ? 1 : 0;
}

// the records with slots [recBase, recBase + n) -> out[slot - recBase]
static __global__ __launch_bounds__(kTPB) void k_paint_records(PaintArgs p, const int32_t *__restrict__ flags, const uint32_t *__restrict__ off,
                                                         uint32_t recBase, uint32_t n, PaintRec *__restrict__ out)
{
  const int f = blockIdx.x * kTPB + threadIdx.x;
  if (f >= p.nFrag || !flags[f]) return;
  const uint32_t at = off[f] - recBase;
  if (off[f] < recBase || at >= n) return;
  const unsigned long long b = p.best[f], s = p.second[f];
  const uint32_t c = p.win[f];
  PaintRec r;
  r.qry = p.w.fragGenome[f] - p.w.genomeBase; r.qSeq = p.fragQSeq[f];
  r.ref = (int32_t)(0xffffffffu - (uint32_t)b); r.idBits = (uint32_t)(b >> 32);
  if (c < (uint32_t)p.w.nCand) { r.refSeq = p.seqBase + p.w.candSeq[c]; r.refStart = p.w.refStart[c]; }      // every flagged fragment has a best head
  else { r.refSeq = -1; r.refStart = -1; }
  r.second = s ? (int32_t)(0xffffffffu - (uint32_t)s) : -1; r.secondBits = (uint32_t)(s >> 32);
  r.genomes = p.genomes[f]; r.reserved = 0;
  out[at] = r;
}

}  // namespace ani
