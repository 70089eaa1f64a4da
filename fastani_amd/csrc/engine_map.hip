// engine_map.hip — mapping and reduction: L1 seed lookup + candidate regions, L2 sliding MinHash, identity filter
// (≙ skch::Map, src/map/include/computeMap.hpp:112-545) and the ANI reducer (≙ cgi::computeCGI,
// src/cgi/include/computeCoreIdentity.hpp:166-298), for one query genome or fused for whole batches / kept fragment sets, with the
// record modes of the reducer (profile, fragment distributions, best hits, bootstrap intervals, paint, synteny).  What works on the finished rows
// (clustering, trees) is engine_graph.hip; the whole-genome sketch estimate is engine_sig.hip.
#include <atomic>
#include <thread>
#include "host/engine.hpp"
#include "kernels/l1.hpp"
#include "kernels/l2.hpp"
#include "kernels/reduce.hpp"
#include "kernels/profile.hpp"
#include "kernels/fragdist.hpp"
#include "kernels/ci.hpp"
#include "kernels/boot.hpp"
#include "kernels/hits.hpp"
#include "kernels/synteny.hpp"
#include "kernels/paint.hpp"

namespace anih {
using namespace ani;

// engine_l2.hip (a unit with its own compiler flags): the codes and simulation kernels of the L2 stage
void launch_l2_codes(unsigned grid, hipStream_t s, const L2FastArgs &fa);
void launch_l2_sim_a(unsigned grid, hipStream_t s, const L2FastArgs &fa, const int32_t *list, const unsigned int *listCount);
void launch_l2_sim_b(unsigned grid, hipStream_t s, const L2FastArgs &fa, const int32_t *list, const unsigned int *listCount);
static_assert(kL1FilterMinHits == 300 && kL1HitCapMax == 4080, "defaults of ani_ctx::l1FilterMin / l1LdsMax (host/engine.hpp)");

// What the L1 half did with the fragments of one call (ani_l1_check reports it; map_stage does not ask)
struct L1Route { unsigned long long tiny = 0, small = 0, mid = 0, big = 0; int attempts = 0; };

// The L1 half of map_stage: processing order, probe, class launches, the pool retry loop, scan and k_l1_order.  The ordered candidates
// stay in ocFrag / ocSeq [chunk-local seqIds] / ocStart / ocEnd; *fragOrderOut is the processing order the L2 half needs (nullptr: ascending).
static int l1_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const FragSet &fs, const int32_t **fragOrderOut, int32_t *nCandOut,
                    L1Route *route = nullptr)
{
  if (ctx->timerPending.size() > 4096) flush_timers(ctx);
  const ani_params_t &p = set->params;
  const int w = p.windowSize, L = p.fragLen;
  const size_t nF = (size_t)fs.nFrag;
  *nCandOut = 0; *fragOrderOut = nullptr;
  if (nF == 0) return ANI_OK;
  unsigned long long host[CNT_N];
  host[CNT_QPOOL] = fs.nHashes;
  ctx->counters.l1Probes += fs.nHashes;

  // ---- processing order ----
  // Fragments are numbered genome by genome.  The genomes of a batch are often close relatives (an all-vs-all run over a species, a
  // database sorted by taxonomy): fragment k of genome A and fragment k of its neighbour B then probe the same index entries, get the
  // same candidates and re-read the same reference ranges.  Processed in fragment order they are a whole genome (1666 workgroups,
  // 200 MB of traffic) apart; processed "k-th fragments of all genomes, then the (k+1)-th" they are neighbours and meet in one L2
  // (kernels map an XCD to a contiguous run of the order, xcd_item).  Results do not depend on the order: every kernel writes through
  // the fragment id, the candidates of a fragment stay contiguous, and single-genome calls (ani_map_query, whose mappings are
  // returned in callback order) keep the ascending order.
  const int32_t *fragOrder = nullptr;
  { const char *ev = getenv("ANI_TEST_FRAG_ORDER");
    if (fs.genomeFragments.size() >= 2 && fs.fragQSeq && !(ev && !strcmp(ev, "plain"))) {
      TRY(ctx->fragOrder.ensure(nF * 4)); TRY(ctx->fragOrderTmp.ensure(nF * 20));
      uint64_t *keyIn = ctx->fragOrderTmp.as<uint64_t>(), *keyOut = keyIn + nF; uint32_t *idxIn = (uint32_t *)(keyOut + nF);
      hipLaunchKernelGGL(k_frag_order_keys, dim3(grid_for(nF)), dim3(256), 0, ctx->stream, fs.fragQSeq, (int32_t)nF, keyIn, idxIn);
      size_t tb = 0;
      int keyBits = 1;                              // keys are running fragment ids inside a genome: 11 bits for 5 Mbp genomes, two 8-bit passes
      { int32_t mx = 0; for (int32_t v : fs.genomeFragments) mx = std::max(mx, v); while (keyBits < 32 && (1ll << keyBits) <= (long long)mx) keyBits++; }
      int rc = ani_sort_pairs_u64_u32(keyIn, keyOut, idxIn, ctx->fragOrder.as<uint32_t>(), nF, keyBits, nullptr, &tb, ctx->stream);
      if (rc == 0) { TRY(ctx->sortTmp.ensure(tb + 256));
        rc = ani_sort_pairs_u64_u32(keyIn, keyOut, idxIn, ctx->fragOrder.as<uint32_t>(), nF, keyBits, ctx->sortTmp.p, &tb, ctx->stream); }
      if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the fragment order failed (%d)", rc);
      fragOrder = ctx->fragOrder.as<int32_t>();
    } }

  // ---- L1 ----
  TRY(ctx->fragCandOff.ensure(nF * 4)); TRY(ctx->fragCandCnt.ensure(nF * 4)); TRY(ctx->fragCandCntClamped.ensure(nF * 4));
  TRY(ctx->fragHits.ensure(nF * 4)); TRY(ctx->fragOrdOff.ensure((nF + 1) * 4));
  TRY(ctx->probeFirst.ensure((fs.poolSize + 1) * 4)); TRY(ctx->probeCnt.ensure((fs.poolSize + 1) * 4));      // indexed like the sketch pool
  // First guess of the candidate pool from the context's running estimate, never beyond what 32-bit candidate ids allow (the limit
  // is an error only when the batch really needs more: the retry below).
  const uint64_t kCandLimit = 0x7fffff00ull;      // whole stripes below 2^31
  // at least 4096 per stripe (4 MB): a few heavy fragments fit without a retry
  uint64_t ccap = std::min<uint64_t>(std::max<uint64_t>((uint64_t)((double)nF * ctx->candPerFrag) + ctx->candPoolMin, ctx->candPoolMin * kPoolStripes),
      kCandLimit);
  const bool smallBatch = nF < 16 * (size_t)kPoolStripes;
  if (smallBatch) ccap = std::min<uint64_t>(std::max<uint64_t>(ccap, ctx->smallBatchCandCap), kCandLimit);
  TRY(ctx->l1MidList.ensure(nF * 4)); TRY(ctx->l1BigList.ensure(nF * 4)); TRY(ctx->l1FragDesc.ensure(nF * sizeof(L1FragDesc)));
  unsigned nMid = 0, nBig = 0; unsigned long long nTiny = 0, nSmall = 0;
  std::vector<int32_t> bigFrags, bigInfo;          // fragments beyond the LDS classes and their (sketch size, seed hits)
  unsigned long long hitsTotal = 0;
  uint32_t probeOverflow = 0;                       // fragments k_l1_probe marked with >= 2^31 seed hits: latched after attempt 0 (the probe runs once)
  for (int attempt = 0;; attempt++) {
    ccap = (uint64_t)stripe_cap(ccap) * kPoolStripes;
    TRY(ctx->candFrag.ensure(ccap * 4)); TRY(ctx->candSeq.ensure(ccap * 4)); TRY(ctx->candStart.ensure(ccap * 4)); TRY(ctx->candEnd.ensure(ccap * 4));
    if (attempt == 0) TRY(zero_counters(ctx));
    // only the candidate pool is redone: k_l1_probe's results (CNT_HITS, CNT_NEG = its overflow marker, the class lists) stay
    else TRY(zero_cursors(ctx, POOL_CAND));
    L1Args a;
    a.qPool = fs.qPool; a.fragOff = fs.fragOff; a.fragS = fs.fragS; a.nFrag = (int32_t)nF;
    a.table = sk->table; a.tableSlots = sk->tableSlots; a.sPos = sk->sPos; a.mSeq = sk->mSeq; a.mWpos = sk->mWpos; a.bucketW = w; a.nIndex = sk->n;
    a.minHitsLUT = set->dMinHits; a.lutMaxS = set->dLutMaxS; a.L = L;
    a.candFrag = ctx->candFrag.as<int32_t>(); a.candSeq = ctx->candSeq.as<int32_t>(); a.candStart = ctx->candStart.as<int32_t>();
    a.candEnd = ctx->candEnd.as<int32_t>();
    a.candCap = stripe_cap(ccap); a.candCount = cur_ptr(ctx, POOL_CAND);
    a.fragCandOff = ctx->fragCandOff.as<uint32_t>(); a.fragCandCnt = ctx->fragCandCnt.as<int32_t>(); a.fragHits = ctx->fragHits.as<int32_t>();
    a.sumHits = cnt_ptr(ctx, CNT_HITS); a.tinyCount = cnt_ptr(ctx, CNT_TINY); a.smallCount = cnt_ptr(ctx, CNT_SMALL);
    a.filterShift = 1; while (a.filterShift < 30 && (1 << a.filterShift) < 2 * L) a.filterShift++;
    a.fragOrder = fragOrder; a.fragDesc = ctx->l1FragDesc.as<L1FragDesc>();
    a.filterMinHits = ctx->l1FilterMin; a.ldsHitCap = ctx->l1LdsMax; a.tinyPath = ctx->l1Tiny ? 1 : 0;
    a.probeFirst = ctx->probeFirst.as<uint32_t>(); a.probeCnt = ctx->probeCnt.as<uint32_t>();
    a.midList = ctx->l1MidList.as<int32_t>(); a.midCount = (unsigned int *)cnt_ptr(ctx, CNT_LISTM);
    a.bigList = ctx->l1BigList.as<int32_t>(); a.bigCount = (unsigned int *)cnt_ptr(ctx, CNT_LISTBIG);
    a.overflowCount = (unsigned int *)cnt_ptr(ctx, CNT_NEG); a.hitLimit = ctx->l1HitLimit;
    {
      StageTimer tm(ctx, &ctx->counters.msL1);
      if (attempt == 0) {
        { StageTimer tk(ctx, &ctx->counters.msL1Probe, 1);
          hipLaunchKernelGGL(k_l1_probe, dim3(pad8((nF + kL1ProbeFrags - 1) / kL1ProbeFrags)), dim3(kTPB), 0, ctx->stream, a); }
        // the probe routed the fragments to their classes: how many of each decides what is launched
        unsigned long long cls[CNT_N];
        TRY(read_counters(ctx, cls));
        nMid = (unsigned)cls[CNT_LISTM]; nBig = (unsigned)cls[CNT_LISTBIG]; nTiny = cls[CNT_TINY]; nSmall = cls[CNT_SMALL];
        ctx->counters.l1TinyFragments += nTiny;
      }
      if (nTiny && ctx->l1Tiny) { StageTimer tk(ctx, &ctx->counters.msL1Tiny, 1);
        hipLaunchKernelGGL(k_l1_tiny, dim3(pad8((nF + kL1TinyFrags - 1) / kL1TinyFrags)), dim3(kTPB), 0, ctx->stream, a); }
      {
        StageTimer tk(ctx, &ctx->counters.msL1Main, 1);
        // the usual case: (nearly) every fragment is of class S, one workgroup per fragment
        if (2 * nSmall >= nF || getenv("ANI_TEST_L1_DENSE"))
          hipLaunchKernelGGL((k_l1<0, kL1HitCapSmall>), dim3(pad8(nF)), dim3(kTPB), 0, ctx->stream, a, (const int32_t *)nullptr);
        else {                                                            // a fragment set against a foreign shard / chunk: class S is the exception, listed
          TRY(ctx->l1SmallList.ensure((nSmall + 1) * 4));
          HIP_TRY(hipMemsetAsync(cnt_ptr(ctx, CNT_LISTL), 0, 8, ctx->stream));
          hipLaunchKernelGGL(k_l1_list, dim3(grid_for(nF, kTPB)), dim3(kTPB), 0, ctx->stream, a, ctx->l1SmallList.as<int32_t>(), (unsigned int *)cnt_ptr(ctx,
              CNT_LISTL));
          if (nSmall) hipLaunchKernelGGL((k_l1<0, kL1HitCapSmall>), dim3((unsigned)nSmall), dim3(kTPB), 0, ctx->stream, a,
              (const int32_t *)ctx->l1SmallList.as<int32_t>());
        }
      }
      if (attempt == 0) {
        if (nBig) {
          bigFrags.resize(nBig); bigInfo.resize(2 * (size_t)nBig);
          TRY(ctx->l1BigV.ensure((size_t)nBig * 8));
          hipLaunchKernelGGL(k_l1_big_info, dim3(grid_for(nBig)), dim3(256), 0, ctx->stream, (const int32_t *)ctx->l1BigList.as<int32_t>(), nBig, fs.fragS,
                             (const int32_t *)ctx->fragHits.as<int32_t>(), ctx->l1BigV.as<int32_t>());
          HIP_TRY(hipMemcpyAsync(bigFrags.data(), ctx->l1BigList.p, (size_t)nBig * 4, hipMemcpyDeviceToHost, ctx->stream));
          HIP_TRY(hipMemcpyAsync(bigInfo.data(), ctx->l1BigV.p, (size_t)nBig * 8, hipMemcpyDeviceToHost, ctx->stream));
          HIP_TRY(hipStreamSynchronize(ctx->stream));
          ctx->counters.l1BigFragments += nBig;
        }
      }
      if (nMid) hipLaunchKernelGGL((k_l1<kL1HitCapSmall, kL1HitCapMid>), dim3(nMid), dim3(kTPB), 0, ctx->stream, a, (const int32_t *)a.midList);
      if (nBig) {
        // Fragments beyond every LDS class, batched (l1.hpp): groups of fragments whose hits fit the key buffers; one 64-bit key per
        // hit = (fragment rank in the group, position rank of the hit), the second field as wide as this chunk's entry count needs —
        // never wider than the (seqId, wpos) fields it replaced: n <= nContigs x longest contig.
        StageTimer tb(ctx, &ctx->counters.msL1Big, 1);
        int shiftRank = 1;
        while (shiftRank < 31 && (1ll << shiftRank) < (long long)sk->n) shiftRank++;
        const uint64_t maxFrags = std::min<uint64_t>(1ull << std::min(20, 64 - shiftRank), ctx->l1BigGroupFrags);
        const uint64_t budget = ctx->l1BigGroupHits;
        for (size_t b0 = 0; b0 < nBig;) {
          size_t b1 = b0; uint64_t hits = 0, hashes = 0, tiles = 0;
          std::vector<uint32_t> sOff{0}, tileFirst{0}; std::vector<uint64_t> hitOff{0};
          while (b1 < nBig && b1 - b0 < maxFrags && (b1 == b0 || hits + (uint64_t)bigInfo[2 * b1 + 1] <= budget)) {
            const uint64_t sz = (uint64_t)std::max(bigInfo[2 * b1], 0), H = (uint64_t)std::max(bigInfo[2 * b1 + 1], 0);
            hashes += sz; hits += H; tiles += (H + kL1BigTileHits - 1) / kL1BigTileHits;
            sOff.push_back((uint32_t)hashes); hitOff.push_back(hits); tileFirst.push_back((uint32_t)tiles);
            b1++;
          }
          const size_t n = b1 - b0;
          if (tiles > 0x7ffffff0ull || hashes > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "group of oversized fragments with %llu seed hits",
              (unsigned long long)hits);
          // group tables: [frag n][sOff n+1][tileFirst n+1] as 32-bit words, then hitOff (64-bit) — one upload
          const size_t w32 = n + 2 * (n + 1), tblBytes = ((w32 * 4 + 7) / 8) * 8 + (n + 1) * 8;
          TRY(ctx->l1BigTbl.ensure(tblBytes)); TRY(ctx->l1BigHash.ensure((hashes ? hashes : 1) * 4));
          TRY(ctx->l1BigHitsA.ensure((hits ? hits : 1) * 8)); TRY(ctx->l1BigHitsB.ensure((hits ? hits : 1) * 8));
          TRY(ctx->l1BigV.ensure((hits ? hits : 1) * 4 + (size_t)nBig * 8));
          uint8_t *hostTbl = nullptr;
          TRY(pinned_buffer(ctx, 2, tblBytes, (void **)&hostTbl));
          uint32_t *h32 = (uint32_t *)hostTbl;
          memcpy(h32, bigFrags.data() + b0, n * 4); memcpy(h32 + n, sOff.data(), (n + 1) * 4); memcpy(h32 + n + (n + 1), tileFirst.data(), (n + 1) * 4);
          memcpy(hostTbl + ((w32 * 4 + 7) / 8) * 8, hitOff.data(), (n + 1) * 8);
          HIP_TRY(hipMemcpyAsync(ctx->l1BigTbl.p, hostTbl, tblBytes, hipMemcpyHostToDevice, ctx->stream));
          L1BigArgs g;
          const uint32_t *d32 = ctx->l1BigTbl.as<uint32_t>();
          g.frag = (const int32_t *)d32; g.sOff = d32 + n; g.tileFirst = d32 + n + (n + 1);
          g.hitOff = (const uint64_t *)(ctx->l1BigTbl.as<uint8_t>() + ((w32 * 4 + 7) / 8) * 8);
          g.hashOff = ctx->l1BigHash.as<int32_t>(); g.keys = ctx->l1BigHitsA.as<uint64_t>(); g.n = (int)n; g.shiftRank = shiftRank;
          hipLaunchKernelGGL(k_l1_big_offsets, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, a, g);
          if (tiles) {
            hipLaunchKernelGGL(k_l1_big_gather, dim3((unsigned)tiles), dim3(kTPB), 0, ctx->stream, a, g);
            int rankBits = 1; while (rankBits < 64 - shiftRank && (1ull << rankBits) < n) rankBits++;
            size_t tbytes = 0;
            int rc = ani_sort_keys_u64_bits(ctx->l1BigHitsA.as<uint64_t>(), ctx->l1BigHitsB.as<uint64_t>(), (size_t)hits, shiftRank + rankBits, nullptr,
                &tbytes, ctx->stream);
            if (rc == 0) { TRY(ctx->sortTmp.ensure(tbytes + 256));
              rc = ani_sort_keys_u64_bits(ctx->l1BigHitsA.as<uint64_t>(), ctx->l1BigHitsB.as<uint64_t>(), (size_t)hits, shiftRank + rankBits, ctx->sortTmp.p,
                &tbytes, ctx->stream); }
            if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of seed hits failed (%d)", rc);
            hipLaunchKernelGGL(k_l1_big_unpack, dim3(grid_for((size_t)hits, 256, 65535)), dim3(256), 0, ctx->stream, ctx->l1BigHitsB.as<uint64_t>(),
                (uint64_t)hits, shiftRank, (const int32_t *)sk->mSeq, (const int32_t *)sk->mWpos);
          }
          g.keys = ctx->l1BigHitsB.as<uint64_t>();
          hipLaunchKernelGGL(k_l1_big_candidates, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, a, g, ctx->l1BigV.as<int>() + 2 * (size_t)nBig);
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipStreamSynchronize(ctx->stream));      // the pinned table and the group buffers are reused by the next group
          b0 = b1;
        }
      }
      {
      hipLaunchKernelGGL(k_clamp_counts, dim3(grid_for(nF)), dim3(256), 0, ctx->stream, (int32_t)nF, ctx->fragCandCnt.as<int32_t>(), fragOrder,
                         ctx->fragCandCntClamped.as<int32_t>());
      }
    }
    HIP_TRY(hipGetLastError());
    TRY(read_counters(ctx, host));
    if (attempt == 0) { hitsTotal = host[CNT_HITS]; probeOverflow = (uint32_t)host[CNT_NEG]; ctx->counters.l1MidFragments += nMid; }
    if (route) route->attempts = attempt + 1;
    if (ctx->poolMaxStripe[POOL_CAND] <= stripe_cap(ccap)) break;
    if (attempt > 2) return fail(ANI_ERR_INTERNAL, "candidate pool did not converge");
    if (ccap >= kCandLimit) return fail(ANI_ERR_LIMIT, "more than 2^31 L1 candidates in one query batch");
    ccap = std::min<uint64_t>((uint64_t)(1.25 * (double)ctx->poolMaxStripe[POOL_CAND] * kPoolStripes) + ctx->candPoolMin, kCandLimit);
  }
  // Size the pool right next time (by the fullest stripe).  Only a batch that fills the stripes evenly says anything about the next
  // one: a handful of fragments sit in a handful of stripes, and "fullest stripe x 64 / fragments" of a one-fragment batch with
  // 1000 candidates would ask for 80 000 candidates per fragment of the next, million-fragment batch (a bogus 2^31 limit error
  // after 34 GB of pool; seen in the parity suite under ANI_TEST_POOL_POISON).  The estimate follows the batches down as well as up.
  if (!smallBatch) {                             // (a one-to-many query of 1666 fragments counts: without its update every call ran the L1 kernels twice)
    const double seen = 1.25 * (double)ctx->poolMaxStripe[POOL_CAND] * kPoolStripes / (double)nF;
    ctx->candSeen[ctx->candSeenAt++ & 31] = seen;
    double mx = 12.0;
    for (double v : ctx->candSeen) mx = std::max(mx, v);
    ctx->candPerFrag = mx;
  // the next small batch starts from what this one needed (bounded: 1 GB of pool)
  } else ctx->smallBatchCandCap = std::min<uint64_t>(grown_cap(ctx->poolMaxStripe[POOL_CAND]), (uint64_t)1 << 26);
  if (route) { route->tiny = nTiny; route->small = nSmall; route->mid = nMid; route->big = nBig; }
  if (probeOverflow != 0)                      // k_l1_probe: hit counts and offsets are 32-bit per fragment
    return fail(ANI_ERR_LIMIT, "%u query fragment(s) have 2^31 or more seed hits in one index chunk (a hash with ~10^9 occurrences: low-complexity / "
                               "repetitive references); use the reference's -s sanity check or a smaller ANI_MAX_INDEX_MINIMIZERS", probeOverflow);
  ctx->counters.seedHits += hitsTotal;
  uint64_t nCand = 0;
  {
    StageTimer tm(ctx, &ctx->counters.msL1);
    TRY(device_scan(ctx, ctx->fragCandCntClamped.as<int32_t>(), ctx->fragOrdOff.as<uint32_t>(), (uint32_t)nF, &nCand));
    if (nCand) {
      TRY(ctx->ocFrag.ensure(nCand * 4)); TRY(ctx->ocSeq.ensure(nCand * 4)); TRY(ctx->ocStart.ensure(nCand * 4)); TRY(ctx->ocEnd.ensure(nCand * 4));
      hipLaunchKernelGGL(k_l1_order, dim3(grid_for(nF)), dim3(256), 0, ctx->stream, ctx->fragCandOff.as<uint32_t>(), ctx->fragCandCntClamped.as<int32_t>(),
                         ctx->fragOrdOff.as<uint32_t>(), fragOrder, (int32_t)nF, ctx->candSeq.as<int32_t>(), ctx->candStart.as<int32_t>(),
                             ctx->candEnd.as<int32_t>(),
                         ctx->ocFrag.as<int32_t>(), ctx->ocSeq.as<int32_t>(), ctx->ocStart.as<int32_t>(), ctx->ocEnd.as<int32_t>());
      HIP_TRY(hipGetLastError());
    }
  }
  *nCandOut = (int32_t)nCand; *fragOrderOut = fragOrder;
  ctx->counters.l1Candidates += nCand;
  return ANI_OK;
}

// The L2 half of map_stage: sliding MinHash and identity for the nCand > 0 ordered candidates l1_stage left; results in
// refStart / idBits / l2Best.
static int l2_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const FragSet &fs, const int32_t *fragOrder, uint64_t nCand)
{
  const ani_params_t &p = set->params;
  const int k = p.kmerSize, w = p.windowSize, L = p.fragLen;
  const size_t nF = (size_t)fs.nFrag;
  const int maxS = fs.maxS;
  unsigned long long host[CNT_N];
  // ---- L2 ----
  TRY(ctx->l2Best.ensure(nCand * 4)); TRY(ctx->l2First.ensure(nCand * 4)); TRY(ctx->l2Last.ensure(nCand * 4));
  TRY(ctx->refStart.ensure(nCand * 4)); TRY(ctx->idBits.ensure(nCand * 4));
  {
    StageTimer tm(ctx, &ctx->counters.msL2);
    TRY(zero_counters(ctx));
    L2Args a;
    a.candFrag = ctx->ocFrag.as<int32_t>(); a.candSeq = ctx->ocSeq.as<int32_t>(); a.candStart = ctx->ocStart.as<int32_t>();
    a.candEnd = ctx->ocEnd.as<int32_t>();
    a.nCand = (int32_t)nCand; a.qPool = fs.qPool; a.fragOff = fs.fragOff; a.fragS = fs.fragS;
    a.mHash = sk->mHash; a.mWpos = sk->mWpos; a.dup = DupLinks{sk->dupList, sk->nDup, sk->dupBits}; a.mWin = sk->mWin; a.posBase = sk->posBase;
    a.posSample = sk->posSample;
    a.contigFirstMin = sk->contigFirstMin;
    { int lg = 0; while ((2 << lg) <= w) lg++; a.rankShift = 21 - std::max(0, lg - 1); }   // w = 24: 2048 buckets over [0, 2^29)
    a.L = L; a.w = w; a.k = k; a.scratch = nullptr; a.laneStride = 0;
    a.outBest = ctx->l2Best.as<int32_t>(); a.outFirst = ctx->l2First.as<int32_t>(); a.outLast = ctx->l2Last.as<int32_t>();
    a.sumEntries = cnt_ptr(ctx, CNT_ENTRIES); a.sumSteps = cnt_ptr(ctx, CNT_STEPS); a.sumQ = cnt_ptr(ctx, CNT_SUMQ);

    // ordered candidate offset per fragment on the host: chunk [c0,c1) -> fragment range
    uint32_t *ordOff = nullptr;
    TRY(pinned_buffer(ctx, 0, nF * 4, (void **)&ordOff));
    HIP_TRY(hipMemcpyAsync(ordOff, ctx->fragOrdOff.p, nF * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    // Chunks of 2^21 candidates, two buffer sets.  Main stream per chunk: ranges -> scan -> length ordering -> codes -> class-A
    // simulation.  Side stream, after the chunk's class-A launch: the few class-B candidates (s in 256..319; their launch is
    // bound by the serial length of one lane, not by throughput) and the collection of the leftovers — they run underneath the
    // next chunk's ranges/codes kernels, which leave the LDS free, instead of extending every chunk by a latency-bound tail.
    const size_t CH = ctx->l2ChunkCandidates;   // candidates per chunk, 2^21 (a chunk whose code entries exceed 2^32 is rejected by the scan)
    for (int p = 0; p < 2; p++) {
      TRY(ctx->l2Ranges[p].ensure(CH * sizeof(L2Range))); TRY(ctx->l2CodeCount[p].ensure(CH * 4)); TRY(ctx->l2CodeOff[p].ensure(CH * 4));
      TRY(ctx->l2SlowFlag[p].ensure(CH * 4)); TRY(ctx->l2ClassList[p].ensure(CH * 4));
      TRY(ctx->l2Order[p].ensure(CH * 4)); TRY(ctx->l2LenHist[p].ensure((kL2LenBuckets + 4) * 4));
    }
    TRY(ctx->l2SlowList.ensure(nCand * 4));
    HIP_TRY(hipMemsetAsync(cnt_ptr(ctx, CNT_NEG), 0, 8, ctx->stream));
    struct SideJoin { ani_ctx *c; ~SideJoin() { (void)hipStreamSynchronize(c->stream2); } } sideJoin{ctx};   // also on the error paths below
    HIP_TRY(hipEventRecord(ctx->evSetDone[0], ctx->stream)); HIP_TRY(hipEventRecord(ctx->evSetDone[1], ctx->stream));   // both sets free, counters zeroed
    HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->evSetDone[1], 0));
    // (measured, round 5: a small job — a rank's shard of a sharded all-vs-all, two chunks — cut into four so that more of the codes
    //  are written beside a simulation: L2 stage 12.9 -> 13.4 ms, profiles/r05y_ab_l2_chunk_auto_sim8.txt; not kept)
    size_t chunk = CH;
    int nChunk = 0;
    for (size_t c0 = 0; c0 < nCand;) {
      const size_t c1 = std::min<size_t>(nCand, c0 + chunk);
      const size_t n = c1 - c0;
      const int p = nChunk & 1;
      HIP_TRY(hipEventSynchronize(ctx->evSetDone[p]));                 // host: set p may be reallocated; (long done: two chunks ago)
      HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->evSetDone[p], 0));
      L2FastArgs fa;
      fa.g = a; fa.c0 = (int32_t)c0; fa.c1 = (int32_t)c1;
      fa.ranges = ctx->l2Ranges[p].as<L2Range>(); fa.codeCount = ctx->l2CodeCount[p].as<int32_t>(); fa.codeOff = ctx->l2CodeOff[p].as<uint32_t>();
      fa.codes = nullptr; fa.slowFlag = ctx->l2SlowFlag[p].as<int32_t>(); fa.fragCandOff = ctx->fragOrdOff.as<uint32_t>(); fa.fragOrder = fragOrder;
      fa.nFrag = (int32_t)nF;
      // fragments that own candidates c0 and c1-1 (ordOff is non-decreasing; fragments without candidates repeat a value)
      const int32_t fA = (int32_t)(std::upper_bound(ordOff, ordOff + nF, (uint32_t)c0) - ordOff) - 1;
      const int32_t fB = (int32_t)(std::upper_bound(ordOff, ordOff + nF, (uint32_t)(c1 - 1)) - ordOff) - 1;
      fa.fragBase = fA;
      { const char *ev = getenv("ANI_TEST_L2_PATH"); fa.allowFast = (ev && !strcmp(ev, "general")) ? 0 : (ev && !strcmp(ev, "classB")) ? 2 : 1; }
      // the 14-bit window links need cmw + 2 < 2^14 (and a window at all)
      if (L - (w - 1) - (k - 1) + 2 > (int)kWinMask || L - (w - 1) - (k - 1) < 1) fa.allowFast = 0;
      {
        StageTimer tk(ctx, &ctx->counters.msL2Ranges, 1);
        hipLaunchKernelGGL(k_l2_ranges, dim3(grid_for(n)), dim3(kTPB), 0, ctx->stream, fa);
      }
      fa.nFragChunk = fB - fA + 1;
      uint64_t nCodes = 0;
      {
        const int rc = device_scan(ctx, fa.codeCount, ctx->l2CodeOff[p].as<uint32_t>(), (uint32_t)n, &nCodes, ctx->l2CodeLimit);
        // very long candidate ranges: smaller chunk, same candidates again
        if (rc == ANI_ERR_LIMIT && n > 1) { chunk = (n + 1) / 2; ctx->counters.l2ChunkHalvings++; continue; }
        TRY(rc);
      }
      TRY(ctx->l2Codes[p].ensure((nCodes + 64) * 2));
      fa.codes = ctx->l2Codes[p].as<uint32_t>();
      if (nCodes) {
        {
          // order the chunk's candidates by code-stream length (longest first) for the simulation
          StageTimer tk(ctx, &ctx->counters.msL2Ranges, 1);
          HIP_TRY(hipMemsetAsync(ctx->l2LenHist[p].p, 0, kL2LenBuckets * 4, ctx->stream));
          // list length for the simulation launch
          HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ctx->l2LenHist[p].as<unsigned int>() + kL2LenBuckets), (int)n, 1, ctx->stream));
          hipLaunchKernelGGL(k_l2_len_hist, dim3(grid_for(n, kTPB, 2048)), dim3(kTPB), 0, ctx->stream, (const L2Range *)fa.ranges, (int32_t)n,
              ctx->l2LenHist[p].as<unsigned int>());
          hipLaunchKernelGGL(k_l2_len_scan, dim3(1), dim3(kTPB), 0, ctx->stream, ctx->l2LenHist[p].as<unsigned int>());
          hipLaunchKernelGGL(k_l2_len_scatter, dim3(grid_for(n, kTPB)), dim3(kTPB), 0, ctx->stream, (const L2Range *)fa.ranges, (int32_t)c0, (int32_t)n,
                             ctx->l2LenHist[p].as<unsigned int>(), ctx->l2Order[p].as<int32_t>());
        }
        {
          StageTimer tk(ctx, &ctx->counters.msL2Codes, 1);
          launch_l2_codes((unsigned)((fa.nFragChunk + 7) / 8 * 8), ctx->stream, fa);
        }
        // The simulation (VALU-bound) runs on the side stream so that the next chunk's ranges / codes kernels (memory- and latency-
        // bound) start beside it; ANI_TEST_L2_OVERLAP=0 keeps everything on the main stream.  Measured (1000 x 1000; round 3:
        // profiles/r03f_bench_overlap.json.log, round 4 A/B/A/B on one box: profiles/r04p_overlap_ab.txt): the L2 stage 91.4 -> 87.8 ms,
        // the step 211.5 -> 207.9 ms — all of it from the tails: a codes workgroup (25 KiB of LDS) does not fit the 16 KiB slot a
        // retiring simulation workgroup frees.  Default since round 4.  With it the per-kernel times (bench line, rocprofv3) are those
        // of kernels that share the machine for part of their run; the stage time (msL2, bracketed on the main stream, which waits for
        // both) is what the headline roofline fraction is computed from.
        const bool overlap = ctx->l2Overlap;
        hipStream_t simStream = ctx->stream;
        if (overlap) {
          HIP_TRY(hipEventRecord(ctx->evSimA[p], ctx->stream));            // codes of this chunk are written
          HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->evSimA[p], 0));
          simStream = ctx->stream2;
        }
        {
          StageTimer tk(ctx, &ctx->counters.msL2Kernel, 1, simStream);
          launch_l2_sim_a(grid_for(n, kL2SimTPB), simStream, fa, (const int32_t *)ctx->l2Order[p].as<int32_t>(),
              (const unsigned int *)ctx->l2LenHist[p].as<unsigned int>() + kL2LenBuckets);
        }
        ctx->counters.l2Launches++;
      }
      HIP_TRY(hipEventRecord(ctx->evSimA[p], ctx->stream));
      HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->evSimA[p], 0));
      if (nCodes) {
        StageTimer tk(ctx, &ctx->counters.msL2SimB, 1, ctx->stream2);
        // class-B candidates are compacted first so that they fill whole waves
        HIP_TRY(hipMemsetAsync(cnt_ptr(ctx, CNT_CLASSB), 0, 8, ctx->stream2));
        hipLaunchKernelGGL(k_l2_collect_class, dim3(grid_for(n)), dim3(256), 0, ctx->stream2, (int32_t)c0, (int32_t)n, (const int32_t *)fa.slowFlag, 4,
                           ctx->l2ClassList[p].as<int32_t>(), (unsigned int *)cnt_ptr(ctx, CNT_CLASSB));
        L2FastArgs fb = fa;       // class B accumulates its algorithmic-byte counters separately
        fb.g.sumEntries = cnt_ptr(ctx, CNT_ENTRIES_B); fb.g.sumQ = cnt_ptr(ctx, CNT_SUMQ_B); fb.g.sumSteps = cnt_ptr(ctx, CNT_STEPS_B);
        launch_l2_sim_b(grid_for(n, kL2SimTPB), ctx->stream2, fb, (const int32_t *)ctx->l2ClassList[p].as<int32_t>(), (const unsigned int *)cnt_ptr(ctx,
            CNT_CLASSB));
      }
      // whatever did not qualify (or overflowed a gap counter) is appended to the sub-batch's list for the general kernel
      hipLaunchKernelGGL(k_l2_collect_slow, dim3(grid_for(n)), dim3(256), 0, ctx->stream2, (int32_t)c0, (int32_t)n, (const int32_t *)fa.slowFlag,
                         ctx->l2SlowList.as<int32_t>(), (unsigned int *)cnt_ptr(ctx, CNT_NEG), cnt_ptr(ctx, CNT_REASON));
      HIP_TRY(hipEventRecord(ctx->evSetDone[p], ctx->stream2));
      HIP_TRY(hipGetLastError());
      c0 = c1; nChunk++;
    }
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->evSetDone[0], 0)); HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->evSetDone[1], 0));
    unsigned long long nSlow64 = 0;
    HIP_TRY(hipMemcpyAsync(&nSlow64, cnt_ptr(ctx, CNT_NEG), 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t nSlowTotal = (size_t)(uint32_t)nSlow64;
    if (nSlowTotal) {
      size_t lanes = (std::min<size_t>(nSlowTotal, (size_t)1 << 17) + kTPB - 1) / kTPB * kTPB;
      const size_t wordsPerLane = (size_t)maxS + 1;
      while (lanes > kTPB && lanes * wordsPerLane * 4 > ((size_t)2 << 30)) lanes = (lanes / 2 + kTPB - 1) / kTPB * kTPB;
      TRY(ctx->l2Scratch.ensure(lanes * wordsPerLane * 4));
      L2Args sa = a; sa.scratch = ctx->l2Scratch.as<uint32_t>(); sa.laneStride = lanes;
      StageTimer tk(ctx, &ctx->counters.msL2Slow, 1);
      for (size_t base = 0; base < nSlowTotal; base += lanes)
        hipLaunchKernelGGL(k_l2, dim3((unsigned)(lanes / kTPB)), dim3(kTPB), 0, ctx->stream, sa, (const int32_t *)ctx->l2SlowList.as<int32_t>(),
            (int32_t)nSlowTotal, (int32_t)base);
      HIP_TRY(hipGetLastError());
    }
    ctx->counters.l2SlowCandidates += nSlowTotal; ctx->counters.l2FastCandidates += nCand - nSlowTotal;
    FinishArgs fa;
    fa.nCand = (int32_t)nCand; fa.candFrag = a.candFrag; fa.candSeq = a.candSeq; fa.best = a.outBest; fa.firstPos = a.outFirst; fa.lastPos = a.outLast;
    fa.fragS = a.fragS; fa.idLUT = set->dIdLUT; fa.minShared = set->dMinShared; fa.lutMaxS = set->dLutMaxS;
    fa.refStart = ctx->refStart.as<int32_t>(); fa.idBits = ctx->idBits.as<uint32_t>();
    hipLaunchKernelGGL(k_finish_candidates, dim3(grid_for(nCand)), dim3(256), 0, ctx->stream, fa);
    HIP_TRY(hipGetLastError());
  }
  TRY(read_counters(ctx, host));
  ctx->counters.l2WindowEntries += host[CNT_ENTRIES] + host[CNT_ENTRIES_B]; ctx->counters.l2Steps += host[CNT_STEPS] + host[CNT_STEPS_B];
  ctx->counters.l2QueryHashes += host[CNT_SUMQ] + host[CNT_SUMQ_B];
  ctx->counters.l2WindowEntriesB += host[CNT_ENTRIES_B]; ctx->counters.l2QueryHashesB += host[CNT_SUMQ_B];
  ctx->counters.l2SlowLimit += host[CNT_REASON + 1]; ctx->counters.l2SlowDup += host[CNT_REASON + 2]; ctx->counters.l2SlowOverflow += host[CNT_REASON + 3];
  return ANI_OK;
}

// L1 + L2 + identity for the fragments of `fs` against ONE index chunk; candidates and their results stay in the context's
// buffers (ocFrag/ocSeq [chunk-local seqIds]/refStart/idBits/l2Best) for the reducer or the mapping export.
int map_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const FragSet &fs, int32_t *nCandOut)
{
  const int32_t *fragOrder = nullptr;
  TRY(l1_stage(ctx, set, sk, fs, &fragOrder, nCandOut));
  if (*nCandOut == 0) return ANI_OK;
  return l2_stage(ctx, set, sk, fs, fragOrder, (uint64_t)*nCandOut);
}

// The fragment distributions of one (sub-batch, index chunk) (kernels/fragdist.hpp), from the bin table and the
// pair table k_pair_reduce has just completed: gate -> flags -> scan -> list, then the records piece by piece (fragDistPiece records
// per launch: the device holds one piece, whatever the number of gated pairs) through page-locked memory into ctx->fdStage, where
// collect_rows finds them.  Only while the sketch has the mode on.
static int fragdist_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const PairArgs &pa)
{
  const size_t nPairs = (size_t)pa.nQuery * (size_t)sk->nGenomes;
  if (nPairs == 0) return ANI_OK;
  FragDistArgs fa;
  fa.nQuery = pa.nQuery; fa.nRefGenomes = sk->nGenomes; fa.bins = pa.bins; fa.binsPerQuery = pa.binsPerQuery; fa.genomeBinStart = sk->genomeBinStart;
  fa.pairCount = pa.pairCount; fa.pairIdentity = pa.pairIdentity; fa.outStride = pa.outStride; fa.outCol0 = pa.outCol0;
  fa.minIdBits = set->fdMinIdBits; fa.minFragments = set->fdMinFragments; fa.genomeBase = sk->g0; fa.nEdges = set->fdEdges;
  memcpy(fa.edgeBits, set->fdEdgeBits, sizeof fa.edgeBits);
  TRY(ctx->fdFlags.ensure(nPairs * 4)); TRY(ctx->fdOff.ensure(nPairs * 4));
  hipLaunchKernelGGL(k_fragdist_flags, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, fa, ctx->fdFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t total = 0;
  TRY(device_scan(ctx, ctx->fdFlags.as<int32_t>(), ctx->fdOff.as<uint32_t>(), (uint32_t)nPairs, &total));
  if (total == 0) return ANI_OK;
  TRY(ctx->fdList.ensure((size_t)total * 4));
  hipLaunchKernelGGL(k_fragdist_list, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, (uint32_t)nPairs, (const int32_t *)ctx->fdFlags.as<int32_t>(),
                     (const uint32_t *)ctx->fdOff.as<uint32_t>(), ctx->fdList.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  const size_t width = (size_t)set->fdEdges + 1, piece = std::min<size_t>(ctx->fragDistPiece, (size_t)total);
  TRY(ctx->fdRec.ensure(piece * sizeof(FragDistRec))); TRY(ctx->fdHist.ensure(piece * width * 4));
  uint8_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, piece * (sizeof(FragDistRec) + width * 4), (void **)&host));
  FragDistBuf &st = ctx->fdStage;
  if (!st.reserve((size_t)total, width)) return fail(ANI_ERR_NOMEM, "host allocation of %llu fragment distribution records failed", (unsigned long long)total);
  static_assert(sizeof(FragDistRec) == sizeof(ani_fragdist_t), "the device record is the ABI's");
  for (size_t first = 0; first < (size_t)total; first += piece) {
    const size_t n = std::min<size_t>(piece, (size_t)total - first);
    hipLaunchKernelGGL(k_fragdist_records, dim3((unsigned)n), dim3(kWave), 0, ctx->stream, fa, (const uint32_t *)ctx->fdList.as<uint32_t>(), (uint32_t)first,
                       (uint32_t)n, ctx->fdRec.as<FragDistRec>(), ctx->fdHist.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, ctx->fdRec.p, n * sizeof(FragDistRec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(host + piece * sizeof(FragDistRec), ctx->fdHist.p, n * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // (into fresh pages: through the host pool, 135 MB of records and histograms per 1000 x 1000 call took one thread longer than the kernels)
    const size_t slice = 4096, at = st.n;
    parallel_for((n + slice - 1) / slice, (uint64_t)n * (sizeof(FragDistRec) + width * 4), [&](size_t i) {
      const size_t r0 = i * slice, m = std::min(slice, n - r0);
      memcpy(st.rec + at + r0, host + r0 * sizeof(FragDistRec), m * sizeof(FragDistRec));
      memcpy(st.hist + (at + r0) * width, host + piece * sizeof(FragDistRec) + r0 * width * 4, m * width * 4);
    });
    st.n += n;
  }
  return ANI_OK;
}

// The staged records of a sub-batch (`in`: chunk by chunk, per chunk queries ascending, per query references ascending) in (query,
// reference) order, appended to `out` with the ids `patch` gives them.  `ordered`: they come from one chunk and are in that order
// already (they are moved, or copied in one piece); else a stable distribution by the query's slot in the sub-batch.
template <class SlotOf, class Patch>
static int fragdist_distribute(FragDistBuf &in, size_t width, size_t nq, bool ordered, SlotOf slot_of, Patch patch, FragDistBuf *out)
{
  const size_t n = in.n;
  if (n == 0) return ANI_OK;
  const size_t at = out->n;
  if (ordered && at == 0) out->swap(in);
  else {
    if (!out->reserve(n, width)) return fail(ANI_ERR_NOMEM, "host allocation of %zu fragment distribution records failed", n);
    if (ordered) { memcpy(out->rec + at, in.rec, n * sizeof(ani_fragdist_t)); memcpy(out->hist + at * width, in.hist, n * width * 4); }
    else {
      std::vector<size_t> start(nq + 1, 0);
      for (size_t r = 0; r < n; r++) start[slot_of(in.rec[r]) + 1]++;
      for (size_t q = 0; q < nq; q++) start[q + 1] += start[q];
      for (size_t r = 0; r < n; r++) {
        const size_t to = at + start[slot_of(in.rec[r])]++;
        out->rec[to] = in.rec[r];
        memcpy(out->hist + to * width, in.hist + r * width, width * 4);
      }
    }
    out->n = at + n;
  }
  for (size_t r = at; r < at + n; r++) patch(out->rec[r]);
  in.clear();
  return ANI_OK;
}

// The best-hit records of one (sub-batch, index chunk) (kernels/hits.hpp), from the bin table, the pair table
// k_pair_reduce has just completed and the candidates k_oneway_bins read: gate -> flags -> scan, owner -> claim over the candidates,
// the list, a second scan over the listed pairs' countSeq for the record offsets, then the records piece by piece (about hitsPiece records
// per launch; a piece ends at a pair border and a larger pair is a piece of its own) through page-locked memory into ctx->hitStage,
// where collect_rows finds them.  Only while the sketch has the mode on.
static int hits_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const OneWayArgs &wa, const PairArgs &pa, const FragSet &fs)
{
  const size_t nPairs = (size_t)pa.nQuery * (size_t)sk->nGenomes, nBins = pa.binsPerQuery * (size_t)pa.nQuery;
  if (nPairs == 0 || wa.nCand == 0 || nBins == 0) return ANI_OK;
  if (!fs.fragQSeq) return fail(ANI_ERR_ARG, "best-hit records need the fragments' querySeqId");
  TRY(ctx->hitOwner.ensure(nBins * 4));                // on top of the bin table: one more uint32 per cell while the mode is on
  HitsArgs ha;
  ha.w = wa; ha.fragQSeq = fs.fragQSeq; ha.nQuery = pa.nQuery; ha.nRefGenomes = sk->nGenomes; ha.genomeBinStart = sk->genomeBinStart;
  ha.pairCount = pa.pairCount; ha.pairIdentity = pa.pairIdentity; ha.outStride = pa.outStride; ha.outCol0 = pa.outCol0;
  ha.minIdBits = set->hitMinIdBits; ha.minFragments = set->hitMinFragments; ha.genomeBase = sk->g0; ha.seqBase = sk->c0;
  ha.owner = ctx->hitOwner.as<uint32_t>();
  TRY(ctx->hitFlags.ensure(nPairs * 4)); TRY(ctx->hitOff.ensure(nPairs * 4));
  hipLaunchKernelGGL(k_hits_flags, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ha, ctx->hitFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t listed = 0, total = 0;
  TRY(device_scan(ctx, ctx->hitFlags.as<int32_t>(), ctx->hitOff.as<uint32_t>(), (uint32_t)nPairs, &listed));
  if (listed == 0) return ANI_OK;
  HIP_TRY(hipMemsetAsync(ctx->hitOwner.p, 0, nBins * 4, ctx->stream));
  hipLaunchKernelGGL(k_hits_owner, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, ha);
  hipLaunchKernelGGL(k_hits_claim, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, ha);
  TRY(ctx->hitList.ensure((size_t)listed * 4)); TRY(ctx->hitCount.ensure((size_t)listed * 4)); TRY(ctx->hitRecOff.ensure((size_t)listed * 4));
  hipLaunchKernelGGL(k_hits_list, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ha, (const int32_t *)ctx->hitFlags.as<int32_t>(),
                     (const uint32_t *)ctx->hitOff.as<uint32_t>(), ctx->hitList.as<uint32_t>(), ctx->hitCount.as<int32_t>());
  HIP_TRY(hipGetLastError());
  // (every record is a candidate of its own, so the sum stays below 2^31; the limit is the ABI's)
  TRY(device_scan(ctx, ctx->hitCount.as<int32_t>(), ctx->hitRecOff.as<uint32_t>(), (uint32_t)listed, &total, 0xfffffff0ull));
  if (total == 0) return ANI_OK;
  std::vector<uint32_t> recOff((size_t)listed + 1);
  HIP_TRY(hipMemcpyAsync(recOff.data(), ctx->hitRecOff.p, (size_t)listed * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  recOff[(size_t)listed] = (uint32_t)total;
  // pieces: [a, b) of the list with recOff[b] - recOff[a] <= hitsPiece, or b = a + 1
  std::vector<size_t> cut(1, 0);
  size_t largest = 0;
  for (size_t a = 0; a < (size_t)listed;) {
    size_t b = a + 1;
    while (b < (size_t)listed && (uint64_t)recOff[b + 1] - recOff[a] <= ctx->hitsPiece) b++;
    largest = std::max<size_t>(largest, recOff[b] - recOff[a]);
    cut.push_back(b); a = b;
  }
  TRY(ctx->hitRec.ensure(largest * sizeof(HitRec)));
  uint8_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, largest * sizeof(HitRec), (void **)&host));
  HitBuf &st = ctx->hitStage;
  if (!st.reserve((size_t)total)) return fail(ANI_ERR_NOMEM, "host allocation of %llu best-hit records failed", (unsigned long long)total);
  static_assert(sizeof(HitRec) == sizeof(ani_hit_t), "the device record is the ABI's");
  for (size_t i = 0; i + 1 < cut.size(); i++) {
    const size_t a = cut[i], b = cut[i + 1], n = recOff[b] - recOff[a];
    hipLaunchKernelGGL(k_hits_records, dim3((unsigned)(b - a)), dim3(kWave), 0, ctx->stream, ha, (const uint32_t *)ctx->hitList.as<uint32_t>(),
                       (const uint32_t *)ctx->hitRecOff.as<uint32_t>(), (uint32_t)a, (uint32_t)(b - a), recOff[a], ctx->hitRec.as<HitRec>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, ctx->hitRec.p, n * sizeof(HitRec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t slice = 8192, at = st.n;
    parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(HitRec), [&](size_t j) {
      const size_t r0 = j * slice, m = std::min(slice, n - r0);
      memcpy(st.rec + at + r0, host + r0 * sizeof(HitRec), m * sizeof(HitRec));
    });
    st.n += n;
  }
  return ANI_OK;
}

// The staged records of a sub-batch (`in`: chunk by chunk, per chunk pairs in (query, reference) order, per pair in bin order) in (query,
// reference) order, appended to `out` with the ids `patch` gives them: fragdist_distribute for groups of any length — the distribution
// by the query's slot is stable, so a pair's records stay together and in their order.
// (the bootstrap intervals' records, one per pair, go the same way)
template <class Rec, class SlotOf, class Patch>
static int hits_distribute(RecBuf<Rec> &in, size_t nq, bool ordered, SlotOf slot_of, Patch patch, RecBuf<Rec> *out)
{
  const size_t n = in.n;
  if (n == 0) return ANI_OK;
  const size_t at = out->n, slice = 65536;
  if (ordered && at == 0) out->swap(in);
  else {
    if (!out->reserve(n)) return fail(ANI_ERR_NOMEM, "host allocation of %zu records failed", n);
    if (ordered) parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(Rec), [&](size_t j) {      // (into fresh pages: see fragdist_stage)
        memcpy(out->rec + at + j * slice, in.rec + j * slice, std::min(slice, n - j * slice) * sizeof(Rec)); });
    else {
      std::vector<size_t> start(nq + 1, 0);
      for (size_t r = 0; r < n; r++) start[slot_of(in.rec[r]) + 1]++;
      for (size_t q = 0; q < nq; q++) start[q + 1] += start[q];
      for (size_t r = 0; r < n; r++) out->rec[at + start[slot_of(in.rec[r])]++] = in.rec[r];
    }
    out->n = at + n;
  }
  parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(Rec), [&](size_t j) {
    for (size_t r = at + j * slice, r1 = at + std::min(n, (j + 1) * slice); r < r1; r++) patch(out->rec[r]); });
  in.clear();
  return ANI_OK;
}

// The bootstrap intervals of one (sub-batch, index chunk) (kernels/ci.hpp), from the bin table and the pair table
// k_pair_reduce has just completed: gate -> flags -> scan -> list, a second scan over the cells the listed pairs keep in the device pool
// (those above the LDS cap), then the records piece by piece — ciPiece records per launch, fewer where the pairs' pool cells exceed 64 per
// record of the piece; a piece ends at a pair border and a larger pair is a piece of its own — through page-locked memory into
// ctx->ciStage, where collect_rows finds them; low and high are computed here.  Only while the sketch has the mode on.
static int ci_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const PairArgs &pa)
{
  const size_t nPairs = (size_t)pa.nQuery * (size_t)sk->nGenomes;
  if (nPairs == 0) return ANI_OK;
  CiArgs ca;
  ca.nQuery = pa.nQuery; ca.nRefGenomes = sk->nGenomes; ca.bins = pa.bins; ca.binsPerQuery = pa.binsPerQuery; ca.genomeBinStart = sk->genomeBinStart;
  ca.pairCount = pa.pairCount; ca.pairIdentity = pa.pairIdentity; ca.outStride = pa.outStride; ca.outCol0 = pa.outCol0;
  ca.minIdBits = set->ciMinIdBits; ca.minFragments = set->ciMinFragments; ca.genomeBase = sk->g0;
  const uint32_t B = set->ciReplicates;
  ca.replicates = B; ca.lowRank = (uint32_t)(((uint64_t)(B - 1) * (1000u - set->ciLevel)) / 2000u); ca.highRank = B - 1 - ca.lowRank; ca.seed = set->ciSeed;
  ca.ldsCells = std::min<uint32_t>(ctx->ciLdsCells, (uint32_t)kCiLdsCells);
  TRY(ctx->ciFlags.ensure(nPairs * 4)); TRY(ctx->ciOff.ensure(nPairs * 4));
  hipLaunchKernelGGL(k_ci_flags, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ca, ctx->ciFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t listed = 0, poolTotal = 0;
  TRY(device_scan(ctx, ctx->ciFlags.as<int32_t>(), ctx->ciOff.as<uint32_t>(), (uint32_t)nPairs, &listed));
  if (listed == 0) return ANI_OK;
  TRY(ctx->ciList.ensure((size_t)listed * 4)); TRY(ctx->ciPoolCells.ensure((size_t)listed * 4)); TRY(ctx->ciPoolOff.ensure((size_t)listed * 4));
  hipLaunchKernelGGL(k_ci_list, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ca, (const int32_t *)ctx->ciFlags.as<int32_t>(),
                     (const uint32_t *)ctx->ciOff.as<uint32_t>(), ctx->ciList.as<uint32_t>(), ctx->ciPoolCells.as<int32_t>());
  HIP_TRY(hipGetLastError());
  // (the pooled cells are cells of the bin table, which holds fewer than 2^32 - 16)
  TRY(device_scan(ctx, ctx->ciPoolCells.as<int32_t>(), ctx->ciPoolOff.as<uint32_t>(), (uint32_t)listed, &poolTotal));
  std::vector<uint32_t> poolOff;                       // only where a pair is above the cap: else every piece is ciPiece records
  if (poolTotal) {
    poolOff.resize((size_t)listed + 1);
    HIP_TRY(hipMemcpyAsync(poolOff.data(), ctx->ciPoolOff.p, (size_t)listed * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    poolOff[(size_t)listed] = (uint32_t)poolTotal;
  }
  const size_t piece = std::min<size_t>(ctx->ciPiece, (size_t)listed);
  const uint64_t poolPiece = (uint64_t)ctx->ciPiece * 64;
  TRY(ctx->ciRec.ensure(piece * sizeof(CiRec)));
  uint8_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, piece * sizeof(CiRec), (void **)&host));
  CiBuf &st = ctx->ciStage;
  if (!st.reserve((size_t)listed)) return fail(ANI_ERR_NOMEM, "host allocation of %llu interval records failed", (unsigned long long)listed);
  static_assert(sizeof(CiRec) == sizeof(ani_ci_t), "the device record is the ABI's");
  for (size_t a = 0; a < (size_t)listed;) {
    size_t b = std::min(a + piece, (size_t)listed);
    uint32_t poolBase = 0; size_t poolCells = 0;
    if (poolTotal) {
      b = a + 1;
      while (b < a + piece && b < (size_t)listed && (uint64_t)poolOff[b + 1] - poolOff[a] <= poolPiece) b++;
      poolBase = poolOff[a]; poolCells = poolOff[b] - poolOff[a];
    }
    const size_t n = b - a;
    TRY(ctx->ciPool.ensure((poolCells ? poolCells : 1) * 4));     // (the stream is idle: the last piece has been copied)
    hipLaunchKernelGGL(k_ci_records, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, ca, (const uint32_t *)ctx->ciList.as<uint32_t>(),
                       (const uint32_t *)ctx->ciPoolOff.as<uint32_t>(), (uint32_t)a, (uint32_t)n, poolBase, ctx->ciPool.as<uint32_t>(), ctx->ciRec.as<CiRec>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, ctx->ciRec.p, n * sizeof(CiRec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t slice = 4096, at = st.n;
    parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(CiRec), [&](size_t i) {      // (into fresh pages: see fragdist_stage)
      const size_t r0 = i * slice, m = std::min(slice, n - r0);
      memcpy(st.rec + at + r0, host + r0 * sizeof(CiRec), m * sizeof(CiRec));
      for (size_t r = at + r0; r < at + r0 + m; r++) {
        ani_ci_t &x = st.rec[r];
        const double den = (double)x.count * 1048576.0;
        x.low = (float)((double)x.lowSum / den); x.high = (float)((double)x.highSum / den);
      }
    });
    st.n += n;
    a = b;
  }
  return ANI_OK;
}

// The bootstrap replicate records of one (sub-batch, index chunk) (kernels/boot.hpp): ci_stage under this mode's
// own gate, B and seed, with the intervals' flag, list and pool buffers (ci_stage, if it ran, has copied its last piece to the host) —
// gate -> flags -> scan -> list, a second scan over the pool cells of the pairs above the LDS cap, then records and sums piece by piece:
// a piece holds at most bootPiece records (by default as many as keep its sums within 2^28 bytes) and at most 64 pool cells per record
// (of at most 2^18 records: the intervals' pool bound, whatever B),
// ends at a pair border, and a larger pair is a piece of its own — through page-locked memory into ctx->bootStage, where collect_rows
// finds them.  Only while the sketch has the mode on.
static int boot_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const PairArgs &pa)
{
  const size_t nPairs = (size_t)pa.nQuery * (size_t)sk->nGenomes;
  if (nPairs == 0) return ANI_OK;
  CiArgs ca;
  ca.nQuery = pa.nQuery; ca.nRefGenomes = sk->nGenomes; ca.bins = pa.bins; ca.binsPerQuery = pa.binsPerQuery; ca.genomeBinStart = sk->genomeBinStart;
  ca.pairCount = pa.pairCount; ca.pairIdentity = pa.pairIdentity; ca.outStride = pa.outStride; ca.outCol0 = pa.outCol0;
  ca.minIdBits = set->bootMinIdBits; ca.minFragments = set->bootMinFragments; ca.genomeBase = sk->g0;
  const size_t B = set->bootReplicates;
  ca.replicates = (uint32_t)B; ca.lowRank = 0; ca.highRank = 0; ca.seed = set->bootSeed;
  ca.ldsCells = std::min<uint32_t>(ctx->bootLdsCells, (uint32_t)kCiLdsCells);
  TRY(ctx->ciFlags.ensure(nPairs * 4)); TRY(ctx->ciOff.ensure(nPairs * 4));
  hipLaunchKernelGGL(k_ci_flags, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ca, ctx->ciFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t listed = 0, poolTotal = 0;
  TRY(device_scan(ctx, ctx->ciFlags.as<int32_t>(), ctx->ciOff.as<uint32_t>(), (uint32_t)nPairs, &listed));
  if (listed == 0) return ANI_OK;
  TRY(ctx->ciList.ensure((size_t)listed * 4)); TRY(ctx->ciPoolCells.ensure((size_t)listed * 4)); TRY(ctx->ciPoolOff.ensure((size_t)listed * 4));
  hipLaunchKernelGGL(k_ci_list, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ca, (const int32_t *)ctx->ciFlags.as<int32_t>(),
                     (const uint32_t *)ctx->ciOff.as<uint32_t>(), ctx->ciList.as<uint32_t>(), ctx->ciPoolCells.as<int32_t>());
  HIP_TRY(hipGetLastError());
  TRY(device_scan(ctx, ctx->ciPoolCells.as<int32_t>(), ctx->ciPoolOff.as<uint32_t>(), (uint32_t)listed, &poolTotal));
  std::vector<uint32_t> poolOff;                       // only where a pair is above the cap: else every piece is `piece` records
  if (poolTotal) {
    poolOff.resize((size_t)listed + 1);
    HIP_TRY(hipMemcpyAsync(poolOff.data(), ctx->ciPoolOff.p, (size_t)listed * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    poolOff[(size_t)listed] = (uint32_t)poolTotal;
  }
  const size_t cap = ctx->bootPiece ? (size_t)ctx->bootPiece : std::max<size_t>(1, ((size_t)1 << 28) / (B * 8));
  const size_t piece = std::min<size_t>(cap, (size_t)listed);
  const uint64_t poolPiece = (uint64_t)std::min<size_t>(cap, (size_t)1 << 18) * 64;      // (the intervals' bound, whatever B)
  TRY(ctx->bootRec.ensure(piece * sizeof(BootRec))); TRY(ctx->bootSums.ensure(piece * B * 8));
  uint8_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, piece * (sizeof(BootRec) + B * 8), (void **)&host));
  BootBuf &st = ctx->bootStage;
  if (!st.reserve((size_t)listed, B)) return fail(ANI_ERR_NOMEM, "host allocation of %llu replicate records failed", (unsigned long long)listed);
  static_assert(sizeof(BootRec) == sizeof(ani_boot_t), "the device record is the ABI's");
  for (size_t a = 0; a < (size_t)listed;) {
    size_t b = std::min(a + piece, (size_t)listed);
    uint32_t poolBase = 0; size_t poolCells = 0;
    if (poolTotal) {
      b = a + 1;
      while (b < a + piece && b < (size_t)listed && (uint64_t)poolOff[b + 1] - poolOff[a] <= poolPiece) b++;
      poolBase = poolOff[a]; poolCells = poolOff[b] - poolOff[a];
    }
    const size_t n = b - a;
    TRY(ctx->ciPool.ensure((poolCells ? poolCells : 1) * 4));     // (the stream is idle: the last piece has been copied)
    hipLaunchKernelGGL(k_boot_records, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, ca, (const uint32_t *)ctx->ciList.as<uint32_t>(),
                       (const uint32_t *)ctx->ciPoolOff.as<uint32_t>(), (uint32_t)a, (uint32_t)n, poolBase, ctx->ciPool.as<uint32_t>(), ctx->bootRec.as<BootRec>(),
                       ctx->bootSums.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, ctx->bootRec.p, n * sizeof(BootRec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(host + piece * sizeof(BootRec), ctx->bootSums.p, n * B * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t slice = 1024, at = st.n;
    parallel_for((n + slice - 1) / slice, (uint64_t)n * (sizeof(BootRec) + B * 8), [&](size_t i) {     // (into fresh pages: see fragdist_stage)
      const size_t r0 = i * slice, m = std::min(slice, n - r0);
      memcpy(st.rec + at + r0, host + r0 * sizeof(BootRec), m * sizeof(BootRec));
      memcpy(st.sums + (at + r0) * B, host + piece * sizeof(BootRec) + r0 * B * 8, m * B * 8);
    });
    st.n += n;
    a = b;
  }
  return ANI_OK;
}

// fragdist_distribute for the replicate records and their sums (`width` = replicates uint64 per record)
template <class SlotOf, class Patch>
static int boot_distribute(BootBuf &in, size_t width, size_t nq, bool ordered, SlotOf slot_of, Patch patch, BootBuf *out)
{
  const size_t n = in.n;
  if (n == 0) return ANI_OK;
  const size_t at = out->n;
  if (ordered && at == 0) out->swap(in);
  else {
    if (!out->reserve(n, width)) return fail(ANI_ERR_NOMEM, "host allocation of %zu replicate records failed", n);
    if (ordered) { memcpy(out->rec + at, in.rec, n * sizeof(ani_boot_t)); memcpy(out->sums + at * width, in.sums, n * width * 8); }
    else {
      std::vector<size_t> start(nq + 1, 0);
      for (size_t r = 0; r < n; r++) start[slot_of(in.rec[r]) + 1]++;
      for (size_t q = 0; q < nq; q++) start[q + 1] += start[q];
      for (size_t r = 0; r < n; r++) {
        const size_t to = at + start[slot_of(in.rec[r])]++;
        out->rec[to] = in.rec[r];
        memcpy(out->sums + to * width, in.sums + r * width, width * 8);
      }
    }
    out->n = at + n;
  }
  for (size_t r = at; r < at + n; r++) patch(out->rec[r]);
  in.clear();
  return ANI_OK;
}

// The partial paint records of one (sub-batch, index chunk) (kernels/paint.hpp), from the candidates k_oneway_bins
// read: best -> second over the candidates, flags -> scan for the mapped fragments' slots, then the records piece by piece (paintPiece
// records per launch and copy) through page-locked memory into ctx->paintStage as one more part, where collect_rows finds them.  Only
// while the sketch has the mode on.
static int paint_stage(ani_ctx *ctx, IndexChunk *sk, const OneWayArgs &wa, const FragSet &fs)
{
  const size_t nF = (size_t)std::max(fs.nFrag, 0);
  if (wa.nCand == 0 || nF == 0) return ANI_OK;
  if (!fs.fragQSeq) return fail(ANI_ERR_ARG, "paint records need the fragments' querySeqId");
  TRY(ctx->paintBest.ensure(nF * 8)); TRY(ctx->paintSecond.ensure(nF * 8)); TRY(ctx->paintGenomes.ensure(nF * 4)); TRY(ctx->paintWin.ensure(nF * 4));
  TRY(ctx->paintFlags.ensure(nF * 4)); TRY(ctx->paintOff.ensure(nF * 4));
  PaintArgs pa;
  pa.w = wa; pa.fragQSeq = fs.fragQSeq; pa.nFrag = (int32_t)nF; pa.genomeBase = sk->g0; pa.seqBase = sk->c0;
  pa.best = ctx->paintBest.as<unsigned long long>(); pa.second = ctx->paintSecond.as<unsigned long long>();
  pa.genomes = ctx->paintGenomes.as<uint32_t>(); pa.win = ctx->paintWin.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(ctx->paintBest.p, 0, nF * 8, ctx->stream)); HIP_TRY(hipMemsetAsync(ctx->paintSecond.p, 0, nF * 8, ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->paintGenomes.p, 0, nF * 4, ctx->stream)); HIP_TRY(hipMemsetAsync(ctx->paintWin.p, 0xff, nF * 4, ctx->stream));
  hipLaunchKernelGGL(k_paint_best, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, pa);
  hipLaunchKernelGGL(k_paint_second, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, pa);
  hipLaunchKernelGGL(k_paint_flags, dim3(grid_for(nF, kTPB)), dim3(kTPB), 0, ctx->stream, pa, ctx->paintFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t total = 0;
  TRY(device_scan(ctx, ctx->paintFlags.as<int32_t>(), ctx->paintOff.as<uint32_t>(), (uint32_t)nF, &total, 0xfffffff0ull));
  if (total == 0) return ANI_OK;
  const size_t piece = std::min<size_t>(ctx->paintPiece, (size_t)total);
  TRY(ctx->paintRec.ensure(piece * sizeof(PaintRec)));
  uint8_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, piece * sizeof(PaintRec), (void **)&host));
  PaintParts &st = ctx->paintStage;
  if (!st.buf.reserve((size_t)total)) return fail(ANI_ERR_NOMEM, "host allocation of %llu paint records failed", (unsigned long long)total);
  static_assert(sizeof(PaintRec) == sizeof(ani_paint_t), "the device record is the ABI's");
  for (size_t first = 0; first < (size_t)total; first += piece) {
    const size_t n = std::min<size_t>(piece, (size_t)total - first);
    hipLaunchKernelGGL(k_paint_records, dim3(grid_for(nF, kTPB)), dim3(kTPB), 0, ctx->stream, pa, (const int32_t *)ctx->paintFlags.as<int32_t>(),
                       (const uint32_t *)ctx->paintOff.as<uint32_t>(), (uint32_t)first, (uint32_t)n, ctx->paintRec.as<PaintRec>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, ctx->paintRec.p, n * sizeof(PaintRec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t slice = 8192, at = st.buf.n;
    parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(PaintRec), [&](size_t j) {      // (into fresh pages: see fragdist_stage)
      const size_t r0 = j * slice, m = std::min(slice, n - r0);
      memcpy(st.buf.rec + at + r0, host + r0 * sizeof(PaintRec), m * sizeof(PaintRec));
    });
    st.buf.n += n;
  }
  st.cut.push_back(st.buf.n);
  return ANI_OK;
}

// The staged parts of a sub-batch (ctx->paintStage) get the rows' ids and move to `out`, behind the parts it holds.
template <class Patch>
static int paint_collect(PaintParts &in, Patch patch, PaintParts *out)
{
  const size_t n = in.buf.n, slice = 65536;
  if (n == 0) { in.clear(); return ANI_OK; }
  parallel_for((n + slice - 1) / slice, (uint64_t)n * sizeof(ani_paint_t), [&](size_t j) {
    for (size_t r = j * slice, r1 = std::min(n, (j + 1) * slice); r < r1; r++) patch(in.buf.rec[r]); });
  const size_t at = out->buf.n;
  if (at == 0 && out->cut.size() == 1) { out->buf.swap(in.buf); out->cut.swap(in.cut); }
  else {
    if (!out->buf.reserve(n)) return fail(ANI_ERR_NOMEM, "host allocation of %zu paint records failed", n);
    memcpy(out->buf.rec + at, in.buf.rec, n * sizeof(ani_paint_t));
    out->buf.n = at + n;
    for (size_t k = 1; k < in.cut.size(); k++) out->cut.push_back(at + in.cut[k]);
  }
  in.clear();
  return ANI_OK;
}

// The parts of ONE sub-batch (one per index chunk that gave it records; the chunks hold disjoint genomes) joined by ani_paint_merge and
// appended to `out`: the one way of the resident and the streamed path.
static int paint_join(PaintParts &parts, PaintBuf *out)
{
  const size_t nParts = parts.cut.size() - 1;
  if (parts.buf.n == 0) { parts.clear(); return ANI_OK; }
  if (nParts == 1 && out->n == 0) { out->swap(parts.buf); parts.clear(); return ANI_OK; }      // one chunk, nothing pending: the buffer itself
  ani_paint_t *acc = nullptr; size_t nAcc = 0;            // nullptr: the first part itself
  const ani_paint_t *cur = parts.buf.rec + parts.cut[0]; size_t nCur = parts.cut[1] - parts.cut[0];
  for (size_t k = 1; k < nParts; k++) {
    ani_paint_t *next = nullptr; size_t nNext = 0;
    const int rc = ani_paint_merge(cur, nCur, parts.buf.rec + parts.cut[k], parts.cut[k + 1] - parts.cut[k], &next, &nNext);
    free(acc);
    if (rc != ANI_OK) return rc;
    acc = next; nAcc = nNext; cur = acc; nCur = nAcc;
  }
  if (nCur) {
    if (!out->reserve(nCur)) { free(acc); return fail(ANI_ERR_NOMEM, "host allocation of %zu paint records failed", nCur); }
    memcpy(out->rec + out->n, cur, nCur * sizeof(ani_paint_t));
    out->n += nCur;
  }
  free(acc);
  parts.clear();
  return ANI_OK;
}

// The synteny records of one (sub-batch, index chunk) (kernels/synteny.hpp): gate -> flags -> scan, the hits' owner
// -> claim passes over the candidates under THIS mode's gate (into ctx->hitOwner: hits_stage, if on, has finished with it on this stream
// and has waited for its last copy), the list with the pairs' hit counts and pool units, two scans for the hit and pool offsets, then
// piece by piece — at most synPiece pairs, 2^22 hits and 2^24 pool units per piece; a piece ends at a pair border and a larger pair is a
// piece of its own — k_syn_pairs, a scan over the piece's block counts, k_syn_compact, and both record lists through page-locked memory
// into ctx->synStage, where collect_rows finds them.  Only while the sketch has the mode on.
static int synteny_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const OneWayArgs &wa, const PairArgs &pa, const FragSet &fs)
{
  const size_t nPairs = (size_t)pa.nQuery * (size_t)sk->nGenomes, nBins = pa.binsPerQuery * (size_t)pa.nQuery;
  if (nPairs == 0 || wa.nCand == 0 || nBins == 0) return ANI_OK;
  if (!fs.fragQSeq) return fail(ANI_ERR_ARG, "synteny records need the fragments' querySeqId");
  TRY(ctx->hitOwner.ensure(nBins * 4));
  SynArgs sa;
  HitsArgs &ha = sa.h;
  ha.w = wa; ha.fragQSeq = fs.fragQSeq; ha.nQuery = pa.nQuery; ha.nRefGenomes = sk->nGenomes; ha.genomeBinStart = sk->genomeBinStart;
  ha.pairCount = pa.pairCount; ha.pairIdentity = pa.pairIdentity; ha.outStride = pa.outStride; ha.outCol0 = pa.outCol0;
  ha.minIdBits = set->synMinIdBits; ha.minFragments = set->synMinFragments; ha.genomeBase = sk->g0; ha.seqBase = sk->c0;
  ha.owner = ctx->hitOwner.as<uint32_t>();
  sa.ldsHits = std::min<uint32_t>(ctx->synLdsHits, (uint32_t)kSynLdsHits);
  TRY(ctx->synFlags.ensure(nPairs * 4)); TRY(ctx->synOff.ensure(nPairs * 4));
  hipLaunchKernelGGL(k_hits_flags, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, ha, ctx->synFlags.as<int32_t>());
  HIP_TRY(hipGetLastError());
  uint64_t listed = 0, total = 0, poolTotal = 0;
  TRY(device_scan(ctx, ctx->synFlags.as<int32_t>(), ctx->synOff.as<uint32_t>(), (uint32_t)nPairs, &listed));
  if (listed == 0) return ANI_OK;
  HIP_TRY(hipMemsetAsync(ctx->hitOwner.p, 0, nBins * 4, ctx->stream));
  hipLaunchKernelGGL(k_hits_owner, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, ha);
  hipLaunchKernelGGL(k_hits_claim, dim3(grid_for((size_t)wa.nCand, kTPB)), dim3(kTPB), 0, ctx->stream, ha);
  const size_t nL = (size_t)listed;
  TRY(ctx->synList.ensure(nL * 4)); TRY(ctx->synCount.ensure(nL * 4)); TRY(ctx->synRecOff.ensure(nL * 4));
  TRY(ctx->synPoolUnits.ensure(nL * 4)); TRY(ctx->synPoolOff.ensure(nL * 4));
  hipLaunchKernelGGL(k_syn_list, dim3(grid_for(nPairs, kTPB)), dim3(kTPB), 0, ctx->stream, sa, (const int32_t *)ctx->synFlags.as<int32_t>(),
                     (const uint32_t *)ctx->synOff.as<uint32_t>(), ctx->synList.as<uint32_t>(), ctx->synCount.as<int32_t>(), ctx->synPoolUnits.as<int32_t>());
  HIP_TRY(hipGetLastError());
  // (every hit is a candidate of its own, so the sum stays below 2^31, and a pair has at most as many blocks; the limit is the ABI's)
  TRY(device_scan(ctx, ctx->synCount.as<int32_t>(), ctx->synRecOff.as<uint32_t>(), (uint32_t)listed, &total, 0xfffffff0ull));
  if (total == 0) return ANI_OK;
  TRY(device_scan(ctx, ctx->synPoolUnits.as<int32_t>(), ctx->synPoolOff.as<uint32_t>(), (uint32_t)listed, &poolTotal));
  std::vector<uint32_t> recOff(nL + 1), poolOff(nL + 1, 0);
  HIP_TRY(hipMemcpyAsync(recOff.data(), ctx->synRecOff.p, nL * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (poolTotal) HIP_TRY(hipMemcpyAsync(poolOff.data(), ctx->synPoolOff.p, nL * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  recOff[nL] = (uint32_t)total; poolOff[nL] = (uint32_t)poolTotal;
  SynBufs &st = ctx->synStage;
  if (!st.pairs.reserve(nL)) return fail(ANI_ERR_NOMEM, "host allocation of %zu synteny records failed", nL);
  static_assert(sizeof(SynRec) == sizeof(ani_synteny_t) && sizeof(SynBlock) == sizeof(ani_synblock_t), "the device records are the ABI's");
  const uint64_t hitsPiece = 1ull << 22, poolPiece = 1ull << 24;
  for (size_t a = 0; a < nL;) {
    size_t b = a + 1;
    while (b < nL && b - a < ctx->synPiece && (uint64_t)recOff[b + 1] - recOff[a] <= hitsPiece && (uint64_t)poolOff[b + 1] - poolOff[a] <= poolPiece) b++;
    const size_t n = b - a, hits = recOff[b] - recOff[a], units = poolOff[b] - poolOff[a];
    TRY(ctx->synRec.ensure(n * sizeof(SynRec))); TRY(ctx->synBlkPool.ensure(hits * sizeof(SynBlock)));
    TRY(ctx->synBlkCount.ensure(n * 4)); TRY(ctx->synBlkOff.ensure(n * 4));
    TRY(ctx->synPool.ensure((units ? units : 1) * 8));          // (the stream is idle: the last piece has been copied)
    hipLaunchKernelGGL(k_syn_pairs, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, sa, (const uint32_t *)ctx->synList.as<uint32_t>(),
                       (const uint32_t *)ctx->synRecOff.as<uint32_t>(), (const uint32_t *)ctx->synPoolOff.as<uint32_t>(), (uint32_t)a, (uint32_t)n,
                       recOff[a], poolOff[a], ctx->synPool.as<unsigned long long>(), ctx->synRec.as<SynRec>(), ctx->synBlkPool.as<SynBlock>(),
                       ctx->synBlkCount.as<int32_t>());
    HIP_TRY(hipGetLastError());
    uint64_t nBlk = 0;
    TRY(device_scan(ctx, ctx->synBlkCount.as<int32_t>(), ctx->synBlkOff.as<uint32_t>(), (uint32_t)n, &nBlk, 0xfffffff0ull));
    if (nBlk == 0 || nBlk > hits) return fail(ANI_ERR_DEVICE, "synteny: %llu blocks from %zu hits", (unsigned long long)nBlk, hits);
    TRY(ctx->synBlk.ensure((size_t)nBlk * sizeof(SynBlock)));
    hipLaunchKernelGGL(k_syn_compact, dim3((unsigned)n), dim3(kTPB), 0, ctx->stream, (const uint32_t *)ctx->synRecOff.as<uint32_t>(), (uint32_t)a,
                       (uint32_t)n, recOff[a], (const int32_t *)ctx->synBlkCount.as<int32_t>(), (const uint32_t *)ctx->synBlkOff.as<uint32_t>(),
                       (const SynBlock *)ctx->synBlkPool.as<SynBlock>(), ctx->synBlk.as<SynBlock>());
    HIP_TRY(hipGetLastError());
    uint8_t *host = nullptr;
    const size_t recBytes = n * sizeof(SynRec), blkBytes = (size_t)nBlk * sizeof(SynBlock);
    TRY(pinned_buffer(ctx, 1, recBytes + blkBytes, (void **)&host));
    HIP_TRY(hipMemcpyAsync(host, ctx->synRec.p, recBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(host + recBytes, ctx->synBlk.p, blkBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!st.blocks.reserve((size_t)nBlk)) return fail(ANI_ERR_NOMEM, "host allocation of %llu synteny block records failed", (unsigned long long)nBlk);
    memcpy(st.pairs.rec + st.pairs.n, host, recBytes);
    memcpy(st.blocks.rec + st.blocks.n, host + recBytes, blkBytes);
    st.pairs.n += n; st.blocks.n += (size_t)nBlk;
    a = b;
  }
  return ANI_OK;
}

// The staged synteny records of a sub-batch (`in`: chunk by chunk, per chunk pairs in (query, reference) order, the blocks in the pairs'
// order) in (query, reference) order, appended to `out` with the ids `patch` gives the pairs: hits_distribute for two lists that stay
// aligned — the pairs are distributed stably by the query's slot, and every pair takes its `blocks` block records with it.
template <class SlotOf, class Patch>
static int syn_distribute(SynBufs &in, size_t nq, bool ordered, SlotOf slot_of, Patch patch, SynBufs *out)
{
  const size_t n = in.pairs.n, nb = in.blocks.n;
  if (n == 0) { in.clear(); return ANI_OK; }
  const size_t at = out->pairs.n, atB = out->blocks.n;
  if (ordered && at == 0 && atB == 0) { out->pairs.swap(in.pairs); out->blocks.swap(in.blocks); }
  else {
    if (!out->pairs.reserve(n) || !out->blocks.reserve(nb)) return fail(ANI_ERR_NOMEM, "host allocation of %zu synteny records failed", n + nb);
    if (ordered) { memcpy(out->pairs.rec + at, in.pairs.rec, n * sizeof(ani_synteny_t)); memcpy(out->blocks.rec + atB, in.blocks.rec, nb * sizeof(ani_synblock_t)); }
    else {
      std::vector<size_t> start(nq + 1, 0), to(n), blkTo(n + 1, 0);
      for (size_t r = 0; r < n; r++) start[slot_of(in.pairs.rec[r]) + 1]++;
      for (size_t q = 0; q < nq; q++) start[q + 1] += start[q];
      for (size_t r = 0; r < n; r++) { to[r] = start[slot_of(in.pairs.rec[r])]++; blkTo[to[r] + 1] = in.pairs.rec[r].blocks; }
      for (size_t r = 0; r < n; r++) blkTo[r + 1] += blkTo[r];                 // by destination: where the pair's blocks begin
      size_t from = 0;
      for (size_t r = 0; r < n; r++) {
        const size_t k = in.pairs.rec[r].blocks;
        out->pairs.rec[at + to[r]] = in.pairs.rec[r];
        memcpy(out->blocks.rec + atB + blkTo[to[r]], in.blocks.rec + from, k * sizeof(ani_synblock_t));
        from += k;
      }
    }
    out->pairs.n = at + n; out->blocks.n = atB + nb;
  }
  for (size_t r = at; r < at + n; r++) patch(out->pairs.rec[r]);
  in.clear();
  return ANI_OK;
}

// 1-way / 2-way / mean (computeCoreIdentity.hpp:214-297) for the candidates map_stage left in the context's buffers, against one
// index chunk; the (count, identity) results go to the chunk's column block of the dense [nQuery][nRefGenomes] table in ctx->rows.
// `compact`: the table holds this chunk's genomes only ([nQuery][chunk genomes]; a streamed set is reduced and read back chunk by chunk)
int reduce_stage(ani_ctx *ctx, ani_sketch *set, IndexChunk *sk, const FragSet &fs, int32_t nCand, int32_t nQuery, bool compact = false)
{
  if (nQuery == 0 || sk->nGenomes == 0) return ANI_OK;
  const size_t binsPerQuery = sk->totalBins;
  const size_t nBins = binsPerQuery * (size_t)nQuery;
  TRY(ctx->bins.ensure((nBins ? nBins : 1) * 4));
  const size_t nPairsAll = (size_t)nQuery * (size_t)(compact ? sk->nGenomes : set->nGenomes);
  TRY(ctx->rows.ensure((nPairsAll ? nPairsAll : 1) * 8));
  hipError_t e1;
  {
  StageTimer tm(ctx, &ctx->counters.msReduce);
  e1 = hipMemsetAsync(ctx->bins.p, 0, (nBins ? nBins : 1) * 4, ctx->stream);
  OneWayArgs a;
  a.nCand = 0;
  if (nCand) {
    a.nCand = nCand; a.candFrag = ctx->ocFrag.as<int32_t>(); a.candSeq = ctx->ocSeq.as<int32_t>(); a.refStart = ctx->refStart.as<int32_t>();
    a.idBits = ctx->idBits.as<uint32_t>(); a.fragGenome = fs.fragGenome; a.genomeBase = fs.genomeBase; a.contigGenome = sk->contigGenome;
    a.contigBinBase = sk->contigBinBase; a.binWidth = set->params.fragLen - 20; a.bins = ctx->bins.as<uint32_t>(); a.binsPerQuery = binsPerQuery;
    hipLaunchKernelGGL(k_oneway_bins, dim3(grid_for((size_t)nCand)), dim3(256), 0, ctx->stream, a);
  }
  PairArgs pa;
  pa.nQuery = nQuery; pa.nRefGenomes = sk->nGenomes; pa.bins = ctx->bins.as<uint32_t>(); pa.binsPerQuery = binsPerQuery;
  pa.genomeBinStart = sk->genomeBinStart; pa.pairCount = ctx->rows.as<uint32_t>(); pa.pairIdentity = ctx->rows.as<uint32_t>() + nPairsAll;
  pa.outStride = compact ? sk->nGenomes : set->nGenomes; pa.outCol0 = compact ? 0 : sk->g0;
  const size_t nPairs = (size_t)nQuery * (size_t)sk->nGenomes;
  hipLaunchKernelGGL(k_pair_reduce, dim3((unsigned)((nPairs + 3) / 4)), dim3(256), 0, ctx->stream, pa);   // one wave per pair
  if (set->profile) {
    // the conservation profile (kernels/profile.hpp): the bin table and the pair table are both complete here and gone with the next
    // sub-batch; reduce_stage runs once per (sub-batch, index chunk), so every pair is added once
    ProfileArgs fa;
    fa.nQuery = nQuery; fa.nRefGenomes = sk->nGenomes; fa.bins = pa.bins; fa.binsPerQuery = binsPerQuery; fa.genomeBinStart = sk->genomeBinStart;
    fa.pairCount = pa.pairCount; fa.pairIdentity = pa.pairIdentity; fa.outStride = pa.outStride; fa.outCol0 = pa.outCol0;
    fa.minIdBits = set->profMinIdBits; fa.minFragments = set->profMinFragments;
    fa.count = sk->profCount; fa.minBits = sk->profMin; fa.maxBits = sk->profMax; fa.sum = sk->profSum; fa.queries = sk->profQueries;
    if (binsPerQuery) hipLaunchKernelGGL(k_profile_bins, dim3(grid_for(binsPerQuery, kTPB)), dim3(kTPB), 0, ctx->stream, fa);
    hipLaunchKernelGGL(k_profile_queries, dim3(grid_for((size_t)sk->nGenomes, kTPB)), dim3(kTPB), 0, ctx->stream, fa);
  }
  if (set->fragdist) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(fragdist_stage(ctx, set, sk, pa));
  }
  if (set->hits) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(hits_stage(ctx, set, sk, a, pa, fs));
  }
  if (set->ci) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(ci_stage(ctx, set, sk, pa));
  }
  if (set->boot) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(boot_stage(ctx, set, sk, pa));
  }
  if (set->paint) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(paint_stage(ctx, sk, a, fs));
  }
  if (set->synteny) {
    HIP_TRY(e1); HIP_TRY(hipGetLastError());
    TRY(synteny_stage(ctx, set, sk, a, pa, fs));
  }
  }
  HIP_TRY(e1); HIP_TRY(hipGetLastError());
  return ANI_OK;
}

// the dense table of a sub-batch (all chunks reduced) -> rows in (query, reference genome) order, appended to `rows`
// (`block`: the table is the compact one of that chunk — reference genome = block->g0 + column)
// (fdOut, hitOut, ciOut: where the sub-batch's fragment distribution, best-hit and interval records go while those modes are on —
// default: the sketch's pending lists; paintOut: where the chunk's part of the paint records waits for the sub-batch's other chunks —
// default: this call has seen every chunk, the parts are joined into the sketch's pending list; synOut: as hitOut, for the synteny records)
int collect_rows(ani_ctx *ctx, ani_sketch *set, const FragSet &fs, int32_t nQuery, int32_t firstQueryId, RowBuf *rows, const IndexChunk *block = nullptr,
    const int32_t *queryIds = nullptr, FragDistBuf *fdOut = nullptr, HitBuf *hitOut = nullptr, CiBuf *ciOut = nullptr, PaintParts *paintOut = nullptr,
    SynBufs *synOut = nullptr, BootBuf *bootOut = nullptr)
{
  const int32_t nCols = block ? block->nGenomes : set->nGenomes, col0 = (block ? block->g0 : 0) + set->refIdBase;
  const size_t nPairs = (size_t)nQuery * (size_t)nCols;
  if (nPairs == 0) return ANI_OK;
  if (set->fragdist) {
    // the records reduce_stage staged come chunk by chunk with the query's index in the sub-batch: the rows' order and ids
    const int32_t base = set->refIdBase;
    TRY(fragdist_distribute(ctx->fdStage, (size_t)set->fdEdges + 1, (size_t)nQuery, block || set->chunks.size() == 1,
        [](const ani_fragdist_t &r) { return (size_t)r.qryGenomeId; },
        [&](ani_fragdist_t &r) { r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base; },
        fdOut ? fdOut : &set->fdPending));
  }
  if (set->hits) {
    const int32_t base = set->refIdBase;
    TRY(hits_distribute(ctx->hitStage, (size_t)nQuery, block || set->chunks.size() == 1,
        [](const ani_hit_t &r) { return (size_t)r.qryGenomeId; },
        [&](ani_hit_t &r) { r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base; },
        hitOut ? hitOut : &set->hitPending));
  }
  if (set->ci) {
    const int32_t base = set->refIdBase;
    TRY(hits_distribute(ctx->ciStage, (size_t)nQuery, block || set->chunks.size() == 1,
        [](const ani_ci_t &r) { return (size_t)r.qryGenomeId; },
        [&](ani_ci_t &r) { r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base; },
        ciOut ? ciOut : &set->ciPending));
  }
  if (set->boot) {
    const int32_t base = set->refIdBase;
    TRY(boot_distribute(ctx->bootStage, (size_t)set->bootReplicates, (size_t)nQuery, block || set->chunks.size() == 1,
        [](const ani_boot_t &r) { return (size_t)r.qryGenomeId; },
        [&](ani_boot_t &r) { r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base; },
        bootOut ? bootOut : &set->bootPending));
  }
  if (set->paint) {
    // per fragment, not per pair: ids first, then (all chunks seen) the join of the chunks' parts
    const int32_t base = set->refIdBase;
    PaintParts own;
    PaintParts *to = paintOut ? paintOut : &own;
    TRY(paint_collect(ctx->paintStage, [&](ani_paint_t &r) {
          r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base;
          if (r.secondGenomeId >= 0) r.secondGenomeId += base; }, to));
    if (!paintOut) TRY(paint_join(own, &set->paintPending));
  }
  if (set->synteny) {
    const int32_t base = set->refIdBase;
    TRY(syn_distribute(ctx->synStage, (size_t)nQuery, block || set->chunks.size() == 1,
        [](const ani_synteny_t &r) { return (size_t)r.qryGenomeId; },
        [&](ani_synteny_t &r) { r.qryGenomeId = firstQueryId + (queryIds ? queryIds[r.qryGenomeId] : r.qryGenomeId); r.refGenomeId += base; },
        synOut ? synOut : &set->synPending));
  }
  uint32_t *dense = nullptr;
  TRY(pinned_buffer(ctx, 1, nPairs * 8 + 8, (void **)&dense));
  HIP_TRY(hipMemcpyAsync(dense, ctx->rows.p, nPairs * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  // rows per query, then every query's rows at their place: both loops on the host pool (round 5: the serial walk over the table was
  // 1.3 ms per sub-batch of the 1000 x 1000 job — the device idle meanwhile — and seconds of the 9 x 10^8 pairs of 90 000 x 10 000)
  std::vector<size_t> qOff((size_t)nQuery + 1, 0);
  parallel_for((size_t)nQuery, (uint64_t)nPairs * 8, [&](size_t qi) {
    const uint32_t *cnt = dense + qi * (size_t)nCols;
    size_t c = 0;
    for (int32_t g = 0; g < nCols; g++) c += cnt[g] != 0;
    qOff[qi + 1] = c;
  });
  for (int32_t qi = 0; qi < nQuery; qi++) qOff[qi + 1] += qOff[qi];
  const size_t m = qOff[nQuery];
  ani_cgi_t *out0 = rows->grow(m);
  if (!out0) return fail(ANI_ERR_NOMEM, "host allocation of %zu result rows failed", m);
  rows->n += m;
  parallel_for((size_t)nQuery, (uint64_t)nPairs * 8, [&](size_t qi) {                       // query ascending, reference ascending
    const uint32_t *cnt = dense + qi * (size_t)nCols, *idb = cnt + nPairs;
    ani_cgi_t *out = out0 + qOff[qi];
    for (int32_t g = 0; g < nCols; g++) {
      if (!cnt[g]) continue;
      ani_cgi_t r; r.refGenomeId = col0 + g; r.qryGenomeId = firstQueryId + (queryIds ? queryIds[qi] : (int32_t)qi); r.countSeq = (int32_t)cnt[g];
      r.totalQueryFragments = fs.genomeFragments[qi];
      memcpy(&r.identity, &idb[g], 4);
      *out++ = r;
    }
  });
  ctx->counters.cgiRows += m;
  return ANI_OK;
}

// Map + reduce for the fragments of `fs` (a whole set or a slice of one) against every index chunk (all resident); rows appended
int map_fragset(ani_ctx *ctx, ani_sketch *sk, const FragSet &fs, int32_t nQuery, int32_t firstQueryId, RowBuf *rows, const int32_t *queryIds = nullptr)
{
  TRY(upload_luts(sk, fs.maxS));
  for (IndexChunk *ch : sk->chunks) {
    int32_t nCand = 0;
    TRY(map_stage(ctx, sk, ch, fs, &nCand));
    TRY(reduce_stage(ctx, sk, ch, fs, nCand, nQuery));
  }
  return collect_rows(ctx, sk, fs, nQuery, firstQueryId, rows, nullptr, queryIds);
}

// Sub-batches of kept fragment sets, mapped against a whole reference set.  A resident set is walked sub-batch by sub-batch (every
// chunk per sub-batch, one dense result table per sub-batch).  A streamed set is walked CHUNK by chunk — build the chunk's index,
// map every sub-batch of every set against it, drop it — so that each chunk is built once per call however many query genomes
// there are (the reference's own loop has the same shape: per reference split, all queries; core_genome_identity.cpp:55-106);
// the rows of a sub-batch then come chunk by chunk and are put back into (query, reference) order at the end.
// queryIds: per genome, relative to firstQueryId (merged sets), else consecutive
struct SubBatch { const ani_fragset *set; int32_t g0, g1, firstQueryId; FragSet v; const int32_t *queryIds; };
int map_fragsets(ani_ctx *ctx, ani_sketch *sk, const std::vector<const ani_fragset *> &sets, const std::vector<int32_t> &firstQueryIds, RowBuf *rows)
{
  std::vector<SubBatch> sub;
  int maxS = 0;
  const uint64_t subFrags = ctx->subBatchFragments;
  for (size_t si = 0; si < sets.size(); si++) {
    const ani_fragset *f = sets[si];
    if (f->device != ctx->device) return fail(ANI_ERR_ARG, "fragment set lives on device %d, context on %d", f->device, ctx->device);
    if (f->params.kmerSize != sk->params.kmerSize || f->params.windowSize != sk->params.windowSize || f->params.fragLen != sk->params.fragLen)
      return fail(ANI_ERR_ARG, "fragment set and sketch were built with different parameters");
    maxS = std::max(maxS, f->fs.maxS);
    const int32_t nG = (int32_t)f->fs.genomeFragments.size();
    int32_t g0 = 0;
    while (g0 < nG) {
      // sub-batches bounded by fragments (2^20), by the bin table of the largest index chunk (8 GiB) and by the dense result table
      int32_t g1 = g0;
      const uint64_t maxQ = std::max<uint64_t>(1, std::min<uint64_t>((ctx->subBatchBinBytes) / (4ull * std::max<uint32_t>(sk->maxChunkBins, 1)),
                                                                 ((uint64_t)2 << 30) / (8ull * (uint64_t)std::max<int32_t>(sk->nGenomes, 1))));
      while (g1 < nG && (g1 == g0 || ((uint64_t)(f->genomeFragStart[g1] - f->genomeFragStart[g0]) < subFrags && (uint64_t)(g1 - g0) < maxQ))) g1++;
      const int64_t fA = f->genomeFragStart[g0], fB = f->genomeFragStart[g1];
      SubBatch sb; sb.set = f; sb.g0 = g0; sb.g1 = g1;
      sb.queryIds = f->genomeQueryId.empty() ? nullptr : f->genomeQueryId.data() + g0;
      sb.firstQueryId = firstQueryIds[si] + (sb.queryIds ? 0 : g0);
      FragSet &v = sb.v;                                       // slice [g0, g1) of the kept set
      v.nFrag = (int32_t)(fB - fA); v.maxS = f->fs.maxS; v.poolSize = f->fs.poolSize;
      v.genomeFragments.assign(f->fs.genomeFragments.begin() + g0, f->fs.genomeFragments.begin() + g1);
      v.qPool = f->fs.qPool; v.genomeBase = g0;
      if (v.nFrag) { v.fragOff = f->fs.fragOff + fA; v.fragS = f->fs.fragS + fA; v.fragGenome = f->fs.fragGenome + fA; v.fragQSeq = f->fs.fragQSeq + fA; }
      v.nHashes = f->fs.nFrag ? (uint64_t)((double)f->fs.nHashes * (double)v.nFrag / (double)f->fs.nFrag) : 0;      // statistics only (l1Probes)
      sub.push_back(std::move(sb));
      g0 = g1;
    }
  }
  if (!sk->streaming) {
    for (const SubBatch &sb : sub) TRY(map_fragset(ctx, sk, sb.v, sb.g1 - sb.g0, sb.firstQueryId, rows, sb.queryIds));
    return ANI_OK;
  }
  TRY(upload_luts(sk, maxS));
  std::vector<RowBuf> part(sub.size());
  std::vector<FragDistBuf> fdPart(sk->fragdist ? sub.size() : 0);       // the fragment distribution records take the rows' way
  std::vector<HitBuf> hitPart(sk->hits ? sub.size() : 0);               // ... and so do the best-hit records
  std::vector<CiBuf> ciPart(sk->ci ? sub.size() : 0);                   // ... and the interval records
  std::vector<BootBuf> bootPart(sk->boot ? sub.size() : 0);              // ... and the replicate records with their sums
  std::vector<PaintParts> paintPart(sk->paint ? sub.size() : 0);        // the paint records: a part per chunk, joined per sub-batch at the end
  std::vector<SynBufs> synPart(sk->synteny ? sub.size() : 0);           // the synteny records take the best-hit records' way
  for (size_t c = 0; c < sk->chunks.size(); c++) {
    TRY(ensure_chunk(sk, c));
    IndexChunk *ch = sk->chunks[c];
    for (size_t i = 0; i < sub.size(); i++) {
      const SubBatch &sb = sub[i];
      int32_t nCand = 0;
      TRY(map_stage(ctx, sk, ch, sb.v, &nCand));
      TRY(reduce_stage(ctx, sk, ch, sb.v, nCand, sb.g1 - sb.g0, true));
      TRY(collect_rows(ctx, sk, sb.v, sb.g1 - sb.g0, sb.firstQueryId, &part[i], ch, sb.queryIds, sk->fragdist ? &fdPart[i] : nullptr,
          sk->hits ? &hitPart[i] : nullptr, sk->ci ? &ciPart[i] : nullptr, sk->paint ? &paintPart[i] : nullptr,
          sk->synteny ? &synPart[i] : nullptr, sk->boot ? &bootPart[i] : nullptr));
    }
  }
  // a sub-batch's rows are (chunk, query, reference)-ordered and a chunk's references all precede the next chunk's: a stable
  // distribution by query — one counting pass, one scatter; the 7.8e7 rows of a 10 000 x 10 000 run are not comparison-sorted —
  // restores (query, reference) order.  The sub-batches are independent of each other (each owns a run of the output), so they go
  // through the host pool side by side (round 6: done one after the other on one thread this was 0.5 of the 5.2 s of a 10 000 x 10 000 step
  // and most of the minute of host time in the mapping calls of 90 000 x 90 000).
  {
    std::vector<size_t> partOff(sub.size() + 1, 0);
    for (size_t i = 0; i < sub.size(); i++) partOff[i + 1] = partOff[i] + part[i].n;
    const size_t total = partOff[sub.size()];
    if (total) {
      ani_cgi_t *out0 = rows->grow(total);
      if (!out0) return fail(ANI_ERR_NOMEM, "host allocation of %zu result rows failed", total);
      parallel_for(sub.size(), (uint64_t)total * sizeof(ani_cgi_t), [&](size_t i) {
        RowBuf &pb = part[i];
        if (!pb.n) return;
        ani_cgi_t *out = out0 + partOff[i];
        const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
        const int32_t *ids = sub[i].queryIds;          // a merged set: the genomes' query ids (ascending), relative to q0; else consecutive
        auto slot_of = [&](int32_t id) -> size_t { return ids ? (size_t)(std::lower_bound(ids, ids + nq, id - q0) - ids) : (size_t)(id - q0); };
        std::vector<size_t> start((size_t)nq + 1, 0);
        for (size_t r = 0; r < pb.n; r++) start[slot_of(pb.p[r].qryGenomeId) + 1]++;
        for (int32_t q = 0; q < nq; q++) start[(size_t)q + 1] += start[(size_t)q];
        for (size_t r = 0; r < pb.n; r++) out[start[slot_of(pb.p[r].qryGenomeId)]++] = pb.p[r];
        free(pb.p); pb.p = nullptr; pb.n = pb.cap = 0;                // host memory of a big run: each part goes back as soon as it is merged
      });
      rows->n += total;
    }
  }
  for (size_t i = 0; i < fdPart.size(); i++) {
    const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
    const int32_t *ids = sub[i].queryIds;
    TRY(fragdist_distribute(fdPart[i], (size_t)sk->fdEdges + 1, (size_t)nq, sk->chunks.size() == 1, [&](const ani_fragdist_t &r) {
          return ids ? (size_t)(std::lower_bound(ids, ids + nq, r.qryGenomeId - q0) - ids) : (size_t)(r.qryGenomeId - q0); },
        [](ani_fragdist_t &) {}, &sk->fdPending));
  }
  for (size_t i = 0; i < hitPart.size(); i++) {
    const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
    const int32_t *ids = sub[i].queryIds;
    TRY(hits_distribute(hitPart[i], (size_t)nq, sk->chunks.size() == 1, [&](const ani_hit_t &r) {
          return ids ? (size_t)(std::lower_bound(ids, ids + nq, r.qryGenomeId - q0) - ids) : (size_t)(r.qryGenomeId - q0); },
        [](ani_hit_t &) {}, &sk->hitPending));
  }
  for (size_t i = 0; i < ciPart.size(); i++) {
    const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
    const int32_t *ids = sub[i].queryIds;
    TRY(hits_distribute(ciPart[i], (size_t)nq, sk->chunks.size() == 1, [&](const ani_ci_t &r) {
          return ids ? (size_t)(std::lower_bound(ids, ids + nq, r.qryGenomeId - q0) - ids) : (size_t)(r.qryGenomeId - q0); },
        [](ani_ci_t &) {}, &sk->ciPending));
  }
  for (size_t i = 0; i < bootPart.size(); i++) {
    const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
    const int32_t *ids = sub[i].queryIds;
    TRY(boot_distribute(bootPart[i], (size_t)sk->bootReplicates, (size_t)nq, sk->chunks.size() == 1, [&](const ani_boot_t &r) {
          return ids ? (size_t)(std::lower_bound(ids, ids + nq, r.qryGenomeId - q0) - ids) : (size_t)(r.qryGenomeId - q0); },
        [](ani_boot_t &) {}, &sk->bootPending));
  }
  for (size_t i = 0; i < paintPart.size(); i++) TRY(paint_join(paintPart[i], &sk->paintPending));
  for (size_t i = 0; i < synPart.size(); i++) {
    const int32_t q0 = sub[i].firstQueryId, nq = sub[i].g1 - sub[i].g0;
    const int32_t *ids = sub[i].queryIds;
    TRY(syn_distribute(synPart[i], (size_t)nq, sk->chunks.size() == 1, [&](const ani_synteny_t &r) {
          return ids ? (size_t)(std::lower_bound(ids, ids + nq, r.qryGenomeId - q0) - ids) : (size_t)(r.qryGenomeId - q0); },
        [](ani_synteny_t &) {}, &sk->synPending));
  }
  return ANI_OK;
}

}  // namespace anih

extern "C" {

int ani_map_cgi_fragset(ani_ctx *ctx, const ani_sketch *skc, const ani_fragset *f, int32_t firstQueryId, ani_cgi_t **out, size_t *m)
{
  return ani_map_cgi_fragsets(ctx, skc, 1, &f, &firstQueryId, out, m);
}

int ani_map_cgi_fragsets(ani_ctx *ctx, const ani_sketch *skc, int32_t nSets, const ani_fragset *const *frags, const int32_t *firstQueryIds, ani_cgi_t **out,
    size_t *m)
{
  if (!ctx || !skc || nSets < 0 || (nSets && (!frags || !firstQueryIds)) || !out || !m) return fail(ANI_ERR_ARG, "null argument");
  for (int32_t i = 0; i < nSets; i++) if (!frags[i]) return fail(ANI_ERR_ARG, "null fragment set %d", i);
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  HIP_TRY(hipSetDevice(ctx->device));
  RowBuf rows;
  std::vector<const ani_fragset *> sets(frags, frags + nSets);
  std::vector<int32_t> firsts(firstQueryIds, firstQueryIds + nSets);
  TRY(map_fragsets(ctx, sk, sets, firsts, &rows));
  *m = rows.n; *out = rows.release();
  if (!*out) return fail(ANI_ERR_NOMEM, "host allocation failed");
  return ANI_OK;
}

int ani_map_query(ani_ctx *ctx, const ani_sketch *skc, const ani_seq_batch_t *query, ani_mapping_t **out, size_t *n, uint64_t *totalQueryFragments)
{
  if (!ctx || !skc || !out || !n) return fail(ANI_ERR_ARG, "null argument");
  TRY(check_batch(query));
  if (query->nGenomes != 1) return fail(ANI_ERR_ARG, "ani_map_query maps exactly one query genome (Map::Map takes one queryno, computeMap.hpp:93)");
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  HIP_TRY(hipSetDevice(ctx->device));
  DeviceBatch db; FragSet fs;
  TRY(upload_batch(ctx, query, 0, 1, &db));
  TRY(fragment_stage(ctx, sk->params, db, &fs));
  TRY(upload_luts(sk, fs.maxS));
  if (totalQueryFragments) *totalQueryFragments = (uint64_t)fs.genomeFragments[0];
  std::vector<ani_mapping_t> maps;
  for (size_t ci = 0; ci < sk->chunks.size(); ci++) {
    IndexChunk *ch = sk->chunks[ci];
    TRY(ensure_chunk(sk, ci));
    int32_t nCand = 0;
    TRY(map_stage(ctx, sk, ch, fs, &nCand));
    if (!nCand) continue;
    const size_t nC = (size_t)nCand;
    TRY(ctx->keepFlags.ensure(nC * 4)); TRY(ctx->keepOff.ensure((nC + 1) * 4));
    hipLaunchKernelGGL(ani::k_keep_flags, dim3(grid_for(nC)), dim3(256), 0, ctx->stream, (int32_t)nC, ctx->idBits.as<uint32_t>(), ctx->keepFlags.as<int32_t>());
    uint64_t nKeep = 0;
    TRY(device_scan(ctx, ctx->keepFlags.as<int32_t>(), ctx->keepOff.as<uint32_t>(), (uint32_t)nC, &nKeep));
    if (!nKeep) continue;
    TRY(ctx->mapOut.ensure(nKeep * 44));
    hipLaunchKernelGGL(ani::k_emit_mappings, dim3(grid_for(nC)), dim3(256), 0, ctx->stream, (int32_t)nC, ctx->ocFrag.as<int32_t>(), ctx->ocSeq.as<int32_t>(),
                       ctx->refStart.as<int32_t>(), ctx->idBits.as<uint32_t>(), ctx->l2Best.as<int32_t>(), fs.fragS,
                       fs.fragQSeq, ctx->keepOff.as<uint32_t>(), sk->params.fragLen, ch->c0, ctx->mapOut.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    const size_t o = maps.size();
    maps.resize(o + nKeep);
    HIP_TRY(hipMemcpyAsync(maps.data() + o, ctx->mapOut.p, nKeep * 44, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  // callback order (fragment, then reference position): every chunk's block is in that order and chunk c's contigs all precede
  // chunk c+1's, so a stable sort by fragment merges the blocks
  if (sk->chunks.size() > 1)
    std::stable_sort(maps.begin(), maps.end(), [](const ani_mapping_t &a, const ani_mapping_t &b) { return a.querySeqId < b.querySeqId; });
  // nucIdentityUpperBound (computeMap.hpp:378-381) is a host scalar per (sketchSize, shared); memoised
  std::unordered_map<uint64_t, float> memo;
  for (auto &m : maps) {
    const uint64_t key = ((uint64_t)(uint32_t)m.sketchSize << 32) | (uint32_t)m.conservedSketches;
    auto it = memo.find(key);
    if (it == memo.end()) {
      float id, ub; ani::stat::identity(m.conservedSketches, m.sketchSize, sk->params.kmerSize, &id, &ub);
      it = memo.emplace(key, ub).first;
    }
    m.nucIdentityUpperBound = it->second;
  }
  ctx->counters.mappings += maps.size();
  return to_host_malloc(maps, out, n);
}

// The reducer over a foreign mapping list: ani_compute_cgi (one query genome, queryFragStart == nullptr) and the test entry point
// ani_reduce_check (nQuery query genomes in one table: the mappings of query q are those with querySeqId in [queryFragStart[q],
// queryFragStart[q + 1]), and its fragments carry fragGenome = fs.genomeBase + q).  fs.genomeFragments and fs.genomeBase are the
// caller's.  The rows keep the sketch's own reference ids, whatever ani_sketch_set_ref_id_base says.
static int reduce_mapping_list(ani_ctx *ctx, ani_sketch *sk, const ani_mapping_t *mappings, size_t n, const int32_t *queryFragStart, int32_t nQuery,
                               FragSet &fs, int32_t firstQueryId, RowBuf *rows)
{
  if (n > 0x7ffffff0ull) return fail(ANI_ERR_LIMIT, "too many mappings");
  // The device reducer expects the mappings of one (fragment, reference genome) next to each other, which is how Map reports
  // them (fragment, then reference position); only input that is not in that order is sorted (on the device, by
  // (querySeqId, refSeqId) with the record index as payload).
  bool ordered = true;
  for (size_t i = 0; i < n; i++) {
    const ani_mapping_t &a = mappings[i];
    if (a.refSeqId < 0 || a.refSeqId >= sk->nContigs) return fail(ANI_ERR_ARG, "mapping %zu refers to contig %d outside the sketch", i, a.refSeqId);
    if (a.refStartPos < 0 || a.refStartPos > sk->contigLen[a.refSeqId]) return fail(ANI_ERR_ARG, "mapping %zu has refStartPos outside its contig", i);
    // the identity bits go through an unsigned atomicMax and a float sum: (0, 100] only, written so that NaN fails
    if (!(a.nucIdentity > 0.0f && a.nucIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "mapping %zu has an identity outside (0, 100]", i);
    if (a.querySeqId < 0) return fail(ANI_ERR_ARG, "mapping %zu has a negative querySeqId", i);
    if (queryFragStart && a.querySeqId >= queryFragStart[nQuery]) return fail(ANI_ERR_ARG, "mapping %zu has querySeqId %d outside the %d fragments of the queries",
        i, a.querySeqId, queryFragStart[nQuery]);
    if (i && (mappings[i - 1].querySeqId > a.querySeqId || (mappings[i - 1].querySeqId == a.querySeqId
        && mappings[i - 1].refSeqId > a.refSeqId))) ordered = false;
  }
  std::vector<uint32_t> ord;
  if (!ordered) {
    ord.resize(n);
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) { keys[i] = ((uint64_t)(uint32_t)mappings[i].querySeqId << 32) | (uint32_t)mappings[i].refSeqId; ord[i] = (uint32_t)i; }
    TRY(ctx->l1BigHitsA.ensure(n * 8)); TRY(ctx->l1BigHitsB.ensure(n * 8)); TRY(ctx->keepFlags.ensure(n * 4)); TRY(ctx->keepOff.ensure(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->l1BigHitsA.p, keys.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->keepFlags.p, ord.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    size_t tb = 0;
    int rc = ani_sort_pairs_u64_u32(ctx->l1BigHitsA.as<uint64_t>(), ctx->l1BigHitsB.as<uint64_t>(), ctx->keepFlags.as<uint32_t>(),
        ctx->keepOff.as<uint32_t>(), n, 64, nullptr, &tb, ctx->stream);
    if (rc == 0) { TRY(ctx->sortTmp.ensure(tb + 256));
      rc = ani_sort_pairs_u64_u32(ctx->l1BigHitsA.as<uint64_t>(), ctx->l1BigHitsB.as<uint64_t>(), ctx->keepFlags.as<uint32_t>(), ctx->keepOff.as<uint32_t>(),
        n, 64, ctx->sortTmp.p, &tb, ctx->stream); }
    if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of mappings failed (%d)", rc);
    HIP_TRY(hipMemcpyAsync(ord.data(), ctx->keepOff.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  // compress querySeqId -> dense fragment index (ascending, so the fragments of a query are consecutive); split the candidate list by
  // index chunk
  const size_t nCh = sk->chunks.size();
  std::vector<std::vector<int32_t>> cFrag(nCh), cSeq(nCh), cStart(nCh); std::vector<std::vector<uint32_t>> cBits(nCh);
  std::vector<int32_t> fragQ;                        // several queries: fragment -> fs.genomeBase + its query
  std::vector<int32_t> fragId;                       // best-hit, paint or synteny records on: fragment -> its querySeqId as given
  int32_t lastQ = -1, f = -1, q = 0;
  size_t chunkOfSeqHint = 0;
  for (size_t i = 0; i < n; i++) {
    const ani_mapping_t &a = mappings[ordered ? i : ord[i]];
    if (a.querySeqId != lastQ || f < 0) {
      f++; lastQ = a.querySeqId;
      if (queryFragStart) { while (a.querySeqId >= queryFragStart[q + 1]) q++; fragQ.push_back(fs.genomeBase + q); }
      if (sk->hits || sk->paint || sk->synteny) fragId.push_back(a.querySeqId);
    }
    size_t c = chunkOfSeqHint;
    while (c + 1 < nCh && a.refSeqId >= sk->chunks[c]->c0 + sk->chunks[c]->nContigs) c++;
    while (c > 0 && a.refSeqId < sk->chunks[c]->c0) c--;
    chunkOfSeqHint = c;
    uint32_t bits; memcpy(&bits, &a.nucIdentity, 4);
    cFrag[c].push_back(f); cSeq[c].push_back(a.refSeqId - sk->chunks[c]->c0); cStart[c].push_back(a.refStartPos); cBits[c].push_back(bits);
  }
  fs.nFrag = f + 1;
  const size_t nF = (size_t)(f + 1);
  TRY(ctx->fragGenome.ensure((nF ? nF : 1) * 4));
  if (nF && queryFragStart) {
    HIP_TRY(hipMemcpyAsync(ctx->fragGenome.p, fragQ.data(), nF * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  } else if (nF) HIP_TRY(hipMemsetAsync(ctx->fragGenome.p, 0, nF * 4, ctx->stream));
  fs.fragGenome = ctx->fragGenome.as<int32_t>();
  if ((sk->hits || sk->paint || sk->synteny) && nF) {
    TRY(ctx->hitQSeq.ensure(nF * 4));
    HIP_TRY(hipMemcpyAsync(ctx->hitQSeq.p, fragId.data(), nF * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    fs.fragQSeq = ctx->hitQSeq.as<int32_t>();
  }
  for (size_t c = 0; c < nCh; c++) {
    const size_t nc = cFrag[c].size();
    if (nc) {
      TRY(ctx->ocFrag.ensure(nc * 4)); TRY(ctx->ocSeq.ensure(nc * 4)); TRY(ctx->refStart.ensure(nc * 4)); TRY(ctx->idBits.ensure(nc * 4));
      HIP_TRY(hipMemcpyAsync(ctx->ocFrag.p, cFrag[c].data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipMemcpyAsync(ctx->ocSeq.p, cSeq[c].data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipMemcpyAsync(ctx->refStart.p, cStart[c].data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipMemcpyAsync(ctx->idBits.p, cBits[c].data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    TRY(reduce_stage(ctx, sk, sk->chunks[c], fs, (int32_t)nc, nQuery));
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // the next chunk reuses the candidate buffers
  }
  const size_t m0 = rows->n, fd0 = sk->fdPending.n, h0 = sk->hitPending.n, ci0 = sk->ciPending.n, pt0 = sk->paintPending.n, sy0 = sk->synPending.pairs.n,
               bt0 = sk->bootPending.n;
  TRY(collect_rows(ctx, sk, fs, nQuery, firstQueryId, rows));
  if (sk->refIdBase) for (size_t i = m0; i < rows->n; i++) rows->p[i].refGenomeId -= sk->refIdBase;      // collect_rows adds it for the batch entry points
  if (sk->refIdBase) for (size_t i = fd0; i < sk->fdPending.n; i++) sk->fdPending.rec[i].refGenomeId -= sk->refIdBase;
  if (sk->refIdBase) for (size_t i = h0; i < sk->hitPending.n; i++) sk->hitPending.rec[i].refGenomeId -= sk->refIdBase;
  if (sk->refIdBase) for (size_t i = ci0; i < sk->ciPending.n; i++) sk->ciPending.rec[i].refGenomeId -= sk->refIdBase;
  if (sk->refIdBase) for (size_t i = bt0; i < sk->bootPending.n; i++) sk->bootPending.rec[i].refGenomeId -= sk->refIdBase;
  if (sk->refIdBase) for (size_t i = sy0; i < sk->synPending.pairs.n; i++) sk->synPending.pairs.rec[i].refGenomeId -= sk->refIdBase;
  if (sk->refIdBase) for (size_t i = pt0; i < sk->paintPending.n; i++) {
    ani_paint_t &r = sk->paintPending.rec[i];
    r.refGenomeId -= sk->refIdBase;
    if (r.secondGenomeId >= 0) r.secondGenomeId -= sk->refIdBase;
  }
  return ANI_OK;
}

int ani_compute_cgi(ani_ctx *ctx, const ani_sketch *skc, const ani_mapping_t *mappings, size_t n, uint64_t totalQueryFragments, int32_t queryFileNo,
                    ani_cgi_t **out, size_t *m)
{
  if (!ctx || !skc || !out || !m || (n && !mappings)) return fail(ANI_ERR_ARG, "null argument");
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  HIP_TRY(hipSetDevice(ctx->device));
  FragSet fs; fs.genomeFragments.assign(1, (int32_t)totalQueryFragments); fs.genomeBase = 0;
  RowBuf rows;
  TRY(reduce_mapping_list(ctx, sk, mappings, n, nullptr, 1, fs, queryFileNo, &rows));
  *m = rows.n; *out = rows.release();
  if (!*out) return fail(ANI_ERR_NOMEM, "host allocation failed");
  return ANI_OK;
}

// TEST INFRASTRUCTURE (declared in host/engine.hpp, not part of include/ani_abi.h, no product code calls it): the reducer in the shape
// the fused path gives it - several query genomes in one bin table, fragGenome values above a non-zero FragSet::genomeBase, the
// pair grid's partial last block - over a synthetic mapping list.  The mappings of query q are those with querySeqId in
// [queryFragStart[q], queryFragStart[q + 1]); the result is the concatenation over q of ani_compute_cgi(mappings of q,
// totalQueryFragments = queryFragStart[q + 1] - queryFragStart[q], queryFileNo = firstQueryId + q).  One reduce_stage per index chunk
// with nQuery and one collect_rows, as map_fragset runs them.  Validates like ani_compute_cgi; a querySeqId outside
// [0, queryFragStart[nQuery]) is ANI_ERR_ARG too.  tests/test_reducer.py holds it to the oracle.
int ani_reduce_check(ani_ctx *ctx, const ani_sketch *skc, const ani_mapping_t *mappings, size_t n, const int32_t *queryFragStart, int32_t nQuery,
                     int32_t genomeBase, int32_t firstQueryId, ani_cgi_t **out, size_t *m)
{
  if (!ctx || !skc || !out || !m || !queryFragStart || (n && !mappings)) return fail(ANI_ERR_ARG, "null argument");
  if (nQuery < 0 || nQuery > 65536) return fail(ANI_ERR_ARG, "ani_reduce_check: %d queries", nQuery);
  if (genomeBase < 0 || genomeBase > 0x7fffffff - nQuery) return fail(ANI_ERR_ARG, "ani_reduce_check: genomeBase %d", genomeBase);
  if (queryFragStart[0] != 0) return fail(ANI_ERR_ARG, "ani_reduce_check: queryFragStart[0] is not 0");
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  HIP_TRY(hipSetDevice(ctx->device));
  FragSet fs; fs.genomeBase = genomeBase;
  for (int32_t q = 0; q < nQuery; q++) {
    if (queryFragStart[q + 1] < queryFragStart[q]) return fail(ANI_ERR_ARG, "ani_reduce_check: queryFragStart is not ascending at %d", q);
    fs.genomeFragments.push_back(queryFragStart[q + 1] - queryFragStart[q]);
  }
  RowBuf rows;
  TRY(reduce_mapping_list(ctx, sk, mappings, n, queryFragStart, nQuery, fs, firstQueryId, &rows));
  *m = rows.n; *out = rows.release();
  if (!*out) return fail(ANI_ERR_NOMEM, "host allocation failed");
  return ANI_OK;
}

// TEST INFRASTRUCTURE (declared in host/engine.hpp, not part of include/ani_abi.h, no product code calls it): the L1 half of map_stage
// (l1_stage above: processing order, k_l1_probe, the class launches, the pool retry loop, the scan, k_l1_order) run once for the kept
// fragment set `f` against index chunk `chunk`, which is made resident as the map path makes it (ensure_chunk) after
// upload_luts(sk, f's maxS).  info = {nFrag, nCand, poolSize, tiny, small, mid, big fragments of this call, attempts of the candidate pool};
// *out = one malloc'ed block of 32-bit words (ani_free releases it), *words long:
//   ocFrag, ocSeq, ocStart, ocEnd [nCand each: what the L2 half would receive], fragHits [nFrag], probeFirst, probeCnt [poolSize each,
//   aligned with the hash pool; 0xffffffff where k_l1_probe wrote nothing].
// A null argument, a chunk that does not exist or cannot be made resident, a fragment set of another context's device or of other
// parameters (k, window, fragLen) are ANI_ERR_ARG; what l1_stage itself reports (ANI_ERR_LIMIT) comes back as it is.
// tests/test_l1.py holds every array to the sequential definition of computeMap.hpp:283-354.
int ani_l1_check(ani_ctx *ctx, const ani_sketch *skc, int32_t chunk, const ani_fragset *f, uint64_t *info, int32_t **out, size_t *words)
{
  if (!ctx || !skc || !f || !info || !out || !words || skc->ctx != ctx) return fail(ANI_ERR_ARG, "ani_l1_check: bad argument");
  if (f->device != ctx->device) return fail(ANI_ERR_ARG, "ani_l1_check: fragment set lives on device %d, context on %d", f->device, ctx->device);
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  if (chunk < 0 || (size_t)chunk >= sk->chunks.size()) return fail(ANI_ERR_ARG, "ani_l1_check: chunk %d of %zu", chunk, sk->chunks.size());
  if (f->params.kmerSize != sk->params.kmerSize || f->params.windowSize != sk->params.windowSize || f->params.fragLen != sk->params.fragLen)
    return fail(ANI_ERR_ARG, "ani_l1_check: fragment set and sketch were built with different parameters");
  HIP_TRY(hipSetDevice(ctx->device));
  const FragSet &fs = f->fs;
  TRY(upload_luts(sk, fs.maxS));
  if (ensure_chunk(sk, (size_t)chunk) != ANI_OK || !sk->chunks[chunk]->resident)
    return fail(ANI_ERR_ARG, "ani_l1_check: the index arrays of chunk %d cannot be made resident", chunk);
  const size_t nF = (size_t)fs.nFrag, nP = (size_t)fs.poolSize;
  // the probe results as l1_stage sizes them, marked where the probe does not write
  TRY(ctx->probeFirst.ensure((nP + 1) * 4)); TRY(ctx->probeCnt.ensure((nP + 1) * 4));
  HIP_TRY(hipMemsetAsync(ctx->probeFirst.p, 0xff, (nP + 1) * 4, ctx->stream)); HIP_TRY(hipMemsetAsync(ctx->probeCnt.p, 0xff, (nP + 1) * 4, ctx->stream));
  const int32_t *fragOrder = nullptr; int32_t nCand = 0; L1Route route;
  TRY(l1_stage(ctx, sk, sk->chunks[chunk], fs, &fragOrder, &nCand, &route));
  const size_t nC = (size_t)nCand, total = 4 * nC + nF + 2 * nP;
  int32_t *host = (int32_t *)malloc((total ? total : 1) * 4);
  if (!host) return fail(ANI_ERR_NOMEM, "host allocation failed");
  hipError_t e = hipSuccess;
  const void *src[7] = {ctx->ocFrag.p, ctx->ocSeq.p, ctx->ocStart.p, ctx->ocEnd.p, ctx->fragHits.p, ctx->probeFirst.p, ctx->probeCnt.p};
  const size_t len[7] = {nC, nC, nC, nC, nF, nP, nP};
  size_t at = 0;
  for (int i = 0; i < 7; i++) {
    if (len[i] && e == hipSuccess) e = hipMemcpyAsync(host + at, src[i], len[i] * 4, hipMemcpyDeviceToHost, ctx->stream);
    at += len[i];
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { free(host); HIP_TRY(e); }
  info[0] = nF; info[1] = nC; info[2] = nP; info[3] = route.tiny; info[4] = route.small; info[5] = route.mid; info[6] = route.big;
  info[7] = (uint64_t)route.attempts;
  *out = host; *words = total;
  return ANI_OK;
}

// TEST INFRASTRUCTURE (declared in host/engine.hpp, not part of include/ani_abi.h, no product code calls it): map_stage's two calls —
// l1_stage and, if it left candidates, l2_stage — run once for the kept fragment set `f` against index chunk `chunk`, prepared and
// checked as ani_l1_check prepares and checks.  info = {nFrag, nCand, and this call's increase of l2FastCandidates, l2SlowCandidates,
// l2SlowLimit, l2SlowDup, l2SlowOverflow, l2Steps, l2WindowEntries, l2QueryHashes, l2WindowEntriesB, l2Launches, l2ChunkHalvings};
// *out = one malloc'ed block of 9 nCand 32-bit words (ani_free releases it):
//   ocFrag, ocSeq, ocStart, ocEnd, l2Best, l2First, l2Last, refStart, idBits [nCand each].
// tests/test_l2.py holds them to the from-scratch definition of computeL2MappedRegions (tests/l2_cases.py).
int ani_l2_check(ani_ctx *ctx, const ani_sketch *skc, int32_t chunk, const ani_fragset *f, uint64_t *info, int32_t **out, size_t *words)
{
  if (!ctx || !skc || !f || !info || !out || !words || skc->ctx != ctx) return fail(ANI_ERR_ARG, "ani_l2_check: bad argument");
  if (f->device != ctx->device) return fail(ANI_ERR_ARG, "ani_l2_check: fragment set lives on device %d, context on %d", f->device, ctx->device);
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  if (chunk < 0 || (size_t)chunk >= sk->chunks.size()) return fail(ANI_ERR_ARG, "ani_l2_check: chunk %d of %zu", chunk, sk->chunks.size());
  if (f->params.kmerSize != sk->params.kmerSize || f->params.windowSize != sk->params.windowSize || f->params.fragLen != sk->params.fragLen)
    return fail(ANI_ERR_ARG, "ani_l2_check: fragment set and sketch were built with different parameters");
  HIP_TRY(hipSetDevice(ctx->device));
  const FragSet &fs = f->fs;
  TRY(upload_luts(sk, fs.maxS));
  if (ensure_chunk(sk, (size_t)chunk) != ANI_OK || !sk->chunks[chunk]->resident)
    return fail(ANI_ERR_ARG, "ani_l2_check: the index arrays of chunk %d cannot be made resident", chunk);
  const ani_counters_t &c = ctx->counters;
  const uint64_t before[11] = {c.l2FastCandidates, c.l2SlowCandidates, c.l2SlowLimit, c.l2SlowDup, c.l2SlowOverflow, c.l2Steps, c.l2WindowEntries,
                               c.l2QueryHashes, c.l2WindowEntriesB, c.l2Launches, c.l2ChunkHalvings};
  const int32_t *fragOrder = nullptr; int32_t nCand = 0;
  TRY(l1_stage(ctx, sk, sk->chunks[chunk], fs, &fragOrder, &nCand));
  if (nCand) TRY(l2_stage(ctx, sk, sk->chunks[chunk], fs, fragOrder, (uint64_t)nCand));
  const size_t nC = (size_t)nCand, total = 9 * nC;
  int32_t *host = (int32_t *)malloc((total ? total : 1) * 4);
  if (!host) return fail(ANI_ERR_NOMEM, "host allocation failed");
  hipError_t e = hipSuccess;
  const void *src[9] = {ctx->ocFrag.p, ctx->ocSeq.p, ctx->ocStart.p, ctx->ocEnd.p, ctx->l2Best.p, ctx->l2First.p, ctx->l2Last.p, ctx->refStart.p,
                        ctx->idBits.p};
  for (int i = 0; i < 9; i++)
    if (nC && e == hipSuccess) e = hipMemcpyAsync(host + i * nC, src[i], nC * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { free(host); HIP_TRY(e); }
  const uint64_t after[11] = {c.l2FastCandidates, c.l2SlowCandidates, c.l2SlowLimit, c.l2SlowDup, c.l2SlowOverflow, c.l2Steps, c.l2WindowEntries,
                              c.l2QueryHashes, c.l2WindowEntriesB, c.l2Launches, c.l2ChunkHalvings};
  info[0] = (uint64_t)fs.nFrag; info[1] = nC;
  for (int i = 0; i < 11; i++) info[2 + i] = after[i] - before[i];
  *out = host; *words = total;
  return ANI_OK;
}

int ani_map_cgi_batch(ani_ctx *ctx, const ani_sketch *skc, const ani_seq_batch_t *queries, int32_t firstQueryId, ani_cgi_t **out, size_t *m)
{
  if (!ctx || !skc || !out || !m) return fail(ANI_ERR_ARG, "null argument");
  TRY(check_batch(queries));
  ani_sketch *sk = const_cast<ani_sketch *>(skc);
  HIP_TRY(hipSetDevice(ctx->device));
  if (sk->streaming) {
    // a streamed reference set is walked chunk by chunk: the fragment sketches of ALL the queries are made first (1.6 MB per 5 Mbp
    // genome) so that every chunk is built once
    ani_fragset *f = nullptr;
    TRY(ani_fragset_build(ctx, &sk->params, queries, &f));
    const int rc = ani_map_cgi_fragset(ctx, sk, f, firstQueryId, out, m);
    ani_fragset_free(f);
    return rc;
  }
  RowBuf rows;
  // sub-batches bounded by fragments (2^20), by the bin table of the largest index chunk (8 GiB) and by the dense result table
  const int L = sk->params.fragLen;
  int32_t g0 = 0;
  while (g0 < queries->nGenomes) {
    int32_t g1 = g0; uint64_t fr = 0;
    const uint64_t maxQ = std::max<uint64_t>(1, std::min<uint64_t>((ctx->subBatchBinBytes) / (4ull * std::max<uint32_t>(sk->maxChunkBins, 1)),
                                                               ((uint64_t)2 << 30) / (8ull * (uint64_t)std::max<int32_t>(sk->nGenomes, 1))));
    while (g1 < queries->nGenomes && (g1 == g0 || (fr < ctx->subBatchFragments && (uint64_t)(g1 - g0) < maxQ))) {
      for (int32_t c = queries->genomeContigStart[g1]; c < queries->genomeContigStart[g1 + 1]; c++) fr += (uint64_t)(queries->contigLen[c] / L);
      g1++;
    }
    DeviceBatch db; FragSet fs;
    TRY(upload_batch(ctx, queries, g0, g1, &db));
    TRY(fragment_stage(ctx, sk->params, db, &fs));          // once per sub-batch, whatever the number of index chunks
    TRY(upload_luts(sk, fs.maxS));
    for (IndexChunk *ch : sk->chunks) {
      int32_t nCand = 0;
      TRY(map_stage(ctx, sk, ch, fs, &nCand));
      TRY(reduce_stage(ctx, sk, ch, fs, nCand, g1 - g0));
    }
    TRY(collect_rows(ctx, sk, fs, g1 - g0, firstQueryId + g0, &rows));
    g0 = g1;
  }
  *m = rows.n; *out = rows.release();
  if (!*out) return fail(ANI_ERR_NOMEM, "host allocation failed");
  return ANI_OK;
}

// ---- conservation profile (ani_abi.h: ani_sketch_profile_begin) ----
// rule 1: the set-global first bin of every contig, from the contig lengths and fragLen alone
static std::vector<uint64_t> profile_bin_start(const ani_sketch *sk)
{
  const int32_t binW = sk->params.fragLen - 20;
  std::vector<uint64_t> start((size_t)sk->nContigs + 1, 0);
  for (int32_t c = 0; c < sk->nContigs; c++) start[(size_t)c + 1] = start[c] + (uint64_t)(sk->contigLen[c] / binW) + 1;
  return start;
}

int ani_sketch_profile_begin(ani_sketch *sk, float minIdentity, int32_t minFragments)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  ani_ctx *ctx = sk->ctx;
  HIP_TRY(hipSetDevice(sk->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  sk->profile = false;
  auto bail = [&](hipError_t e, const char *what) {
    for (IndexChunk *ch : sk->chunks) free_chunk_profile(ch);
    return fail(e == hipErrorOutOfMemory ? ANI_ERR_NOMEM : ANI_ERR_DEVICE, "profile accumulators: %s failed: %s", what, hipGetErrorString(e));
  };
  for (IndexChunk *ch : sk->chunks) {
    free_chunk_profile(ch);
    const size_t nb = ch->totalBins ? ch->totalBins : 1, ng = ch->nGenomes > 0 ? (size_t)ch->nGenomes : 1;
    hipError_t e;
    if ((e = pool_malloc((void **)&ch->profCount, nb * 4)) != hipSuccess || (e = pool_malloc((void **)&ch->profMin, nb * 4)) != hipSuccess
        || (e = pool_malloc((void **)&ch->profMax, nb * 4)) != hipSuccess || (e = pool_malloc((void **)&ch->profSum, nb * 8)) != hipSuccess
        || (e = pool_malloc((void **)&ch->profQueries, ng * 4)) != hipSuccess) return bail(e, "allocation");
    if ((e = hipMemsetAsync(ch->profCount, 0, nb * 4, ctx->stream)) != hipSuccess || (e = hipMemsetAsync(ch->profMin, 0xff, nb * 4, ctx->stream)) != hipSuccess
        || (e = hipMemsetAsync(ch->profMax, 0, nb * 4, ctx->stream)) != hipSuccess || (e = hipMemsetAsync(ch->profSum, 0, nb * 8, ctx->stream)) != hipSuccess
        || (e = hipMemsetAsync(ch->profQueries, 0, ng * 4, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
  }
  { const hipError_t e = hipStreamSynchronize(ctx->stream); if (e != hipSuccess) return bail(e, "hipStreamSynchronize"); }
  memcpy(&sk->profMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->profMinIdBits = 0;                 // -0.0 counts as 0
  sk->profMinFragments = (uint32_t)minFragments;
  sk->profile = true;
  return ANI_OK;
}

int ani_sketch_profile_bins(const ani_sketch *sk, uint64_t *nBins)
{
  if (!sk || !nBins) return fail(ANI_ERR_ARG, "null argument");
  *nBins = profile_bin_start(sk).back();
  return ANI_OK;
}

int ani_sketch_profile_read(const ani_sketch *sk, ani_binprofile_t *bins, uint32_t *queries)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->profile) return fail(ANI_ERR_ARG, "ani_sketch_profile_read without ani_sketch_profile_begin");
  ani_ctx *ctx = sk->ctx;
  HIP_TRY(hipSetDevice(sk->device));
  const std::vector<uint64_t> binStart = profile_bin_start(sk);
  bool full = false;
  constexpr size_t kPiece = (size_t)1 << 20;                    // bins per staged piece: 20 MB page-locked
  for (const IndexChunk *ch : sk->chunks) {
    if (queries && ch->nGenomes > 0) {
      uint32_t *host = nullptr;
      TRY(pinned_buffer(ctx, 1, (size_t)ch->nGenomes * 4, (void **)&host));
      HIP_TRY(hipMemcpyAsync(host, ch->profQueries, (size_t)ch->nGenomes * 4, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      for (int32_t g = 0; g < ch->nGenomes; g++) { queries[ch->g0 + g] = host[g]; full |= host[g] == kProfileFull; }
    }
    ani_binprofile_t *out = bins ? bins + binStart[ch->c0] : nullptr;
    for (size_t b0 = 0; b0 < ch->totalBins; b0 += kPiece) {
      const size_t n = std::min<size_t>(kPiece, ch->totalBins - b0);
      uint8_t *host = nullptr;
      TRY(pinned_buffer(ctx, 1, n * 20, (void **)&host));
      const uint32_t *hc = (const uint32_t *)(host + n * 8), *hmn = hc + n, *hmx = hmn + n; const unsigned long long *hs = (const unsigned long long *)host;
      HIP_TRY(hipMemcpyAsync(host, ch->profSum + b0, n * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipMemcpyAsync(host + n * 8, ch->profCount + b0, n * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (bins) {
        HIP_TRY(hipMemcpyAsync(host + n * 12, ch->profMin + b0, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(host + n * 16, ch->profMax + b0, n * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      for (size_t i = 0; i < n; i++) {
        full |= hc[i] == kProfileFull;
        if (!out) continue;
        ani_binprofile_t r; r.count = hc[i]; r.reserved = 0; r.sum = hs[i];
        const uint32_t mn = hc[i] ? hmn[i] : 0u, mx = hc[i] ? hmx[i] : 0u;      // the `min` of an empty bin is the sentinel on the device
        memcpy(&r.minIdentity, &mn, 4); memcpy(&r.maxIdentity, &mx, 4);
        out[b0 + i] = r;
      }
    }
  }
  if (full) return fail(ANI_ERR_LIMIT, "a counter of the profile has reached 2^32 - 1");
  return ANI_OK;
}

int ani_sketch_profile_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->profile) return fail(ANI_ERR_ARG, "ani_sketch_profile_end without ani_sketch_profile_begin");
  HIP_TRY(hipSetDevice(sk->device));
  HIP_TRY(hipStreamSynchronize(sk->ctx->stream));        // a reduce_stage of an earlier call may still be adding
  for (IndexChunk *ch : sk->chunks) free_chunk_profile(ch);
  sk->profile = false;
  return ANI_OK;
}

// ---- fragment identity distributions (ani_abi.h: ani_sketch_fragdist_begin) ----
int ani_sketch_fragdist_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, const float *edges, int32_t nEdges)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  if (nEdges < 0 || nEdges > kFragDistMaxEdges) return fail(ANI_ERR_ARG, "%d class edges: 0 to %d are taken", nEdges, kFragDistMaxEdges);
  if (nEdges > 0 && !edges) return fail(ANI_ERR_ARG, "null edges");
  uint32_t eb[kFragDistMaxEdges] = {0};
  for (int32_t e = 0; e < nEdges; e++) {
    if (!(edges[e] >= 0.0f && edges[e] <= 100.0f)) return fail(ANI_ERR_ARG, "edge %d (%g) outside [0, 100]", e, (double)edges[e]);
    if (e && !(edges[e] > edges[e - 1])) return fail(ANI_ERR_ARG, "edge %d (%g) is not above its predecessor", e, (double)edges[e]);
    if (edges[e] != 0.0f) memcpy(&eb[e], &edges[e], 4);            // -0.0 counts as 0
  }
  memcpy(&sk->fdMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->fdMinIdBits = 0;                    // -0.0 counts as 0
  sk->fdMinFragments = (uint32_t)minFragments;
  sk->fdEdges = nEdges; memcpy(sk->fdEdgeBits, eb, sizeof eb);
  sk->fdPending.clear(); sk->ctx->fdStage.clear();
  sk->fragdist = true;
  return ANI_OK;
}

int ani_sketch_fragdist_take(ani_sketch *sk, ani_fragdist_t **rec, uint32_t **hist, size_t *n)
{
  if (!sk || !rec || !n) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->fragdist) return fail(ANI_ERR_ARG, "ani_sketch_fragdist_take without ani_sketch_fragdist_begin");
  *rec = nullptr; *n = 0;
  if (hist) *hist = nullptr;
  FragDistBuf &pd = sk->fdPending;
  if (pd.n == 0) { pd.clear(); return ANI_OK; }
  *rec = pd.rec; *n = pd.n;                     // the buffers themselves: ani_free releases them
  if (hist) *hist = pd.hist; else free(pd.hist);
  pd.rec = nullptr; pd.hist = nullptr; pd.n = pd.cap = 0;
  return ANI_OK;
}

int ani_sketch_fragdist_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->fragdist) return fail(ANI_ERR_ARG, "ani_sketch_fragdist_end without ani_sketch_fragdist_begin");
  sk->fdPending.clear(); sk->ctx->fdStage.clear();
  sk->fragdist = false;
  return ANI_OK;
}

// ---- reciprocal best-hit records (ani_abi.h: ani_sketch_hits_begin) ----
int ani_sketch_hits_begin(ani_sketch *sk, float minIdentity, int32_t minFragments)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  memcpy(&sk->hitMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->hitMinIdBits = 0;                   // -0.0 counts as 0
  sk->hitMinFragments = (uint32_t)minFragments;
  sk->hitPending.clear(); sk->ctx->hitStage.clear();
  sk->hits = true;
  return ANI_OK;
}

int ani_sketch_hits_take(ani_sketch *sk, ani_hit_t **rec, size_t *n)
{
  if (!sk || !rec || !n) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->hits) return fail(ANI_ERR_ARG, "ani_sketch_hits_take without ani_sketch_hits_begin");
  *rec = nullptr; *n = 0;
  HitBuf &pd = sk->hitPending;
  if (pd.n == 0) { pd.clear(); return ANI_OK; }
  *rec = pd.rec; *n = pd.n;                     // the buffer itself: ani_free releases it
  pd.rec = nullptr; pd.n = pd.cap = 0;
  return ANI_OK;
}

int ani_sketch_hits_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->hits) return fail(ANI_ERR_ARG, "ani_sketch_hits_end without ani_sketch_hits_begin");
  sk->hitPending.clear(); sk->ctx->hitStage.clear();
  sk->hits = false;
  return ANI_OK;
}

// ---- bootstrap intervals of the ANI values (ani_abi.h: ani_sketch_ci_begin) ----
int ani_sketch_ci_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, int32_t replicates, int32_t levelPermille, uint32_t seed)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  if (replicates < 1 || replicates > kCiMaxReplicates) return fail(ANI_ERR_ARG, "%d replicates: 1 to %d are taken", replicates, kCiMaxReplicates);
  if (levelPermille < 1 || levelPermille > 999) return fail(ANI_ERR_ARG, "level %d permille outside 1 .. 999", levelPermille);
  memcpy(&sk->ciMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->ciMinIdBits = 0;                    // -0.0 counts as 0
  sk->ciMinFragments = (uint32_t)minFragments;
  sk->ciReplicates = (uint32_t)replicates; sk->ciLevel = (uint32_t)levelPermille; sk->ciSeed = seed;
  sk->ciPending.clear(); sk->ctx->ciStage.clear();
  sk->ci = true;
  return ANI_OK;
}

int ani_sketch_ci_take(ani_sketch *sk, ani_ci_t **rec, size_t *n)
{
  if (!sk || !rec || !n) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->ci) return fail(ANI_ERR_ARG, "ani_sketch_ci_take without ani_sketch_ci_begin");
  *rec = nullptr; *n = 0;
  CiBuf &pd = sk->ciPending;
  if (pd.n == 0) { pd.clear(); return ANI_OK; }
  *rec = pd.rec; *n = pd.n;                     // the buffer itself: ani_free releases it
  pd.rec = nullptr; pd.n = pd.cap = 0;
  return ANI_OK;
}

int ani_sketch_ci_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->ci) return fail(ANI_ERR_ARG, "ani_sketch_ci_end without ani_sketch_ci_begin");
  sk->ciPending.clear(); sk->ctx->ciStage.clear();
  sk->ci = false;
  return ANI_OK;
}

// ---- bootstrap replicate records (ani_abi.h: ani_sketch_boot_begin) ----
int ani_sketch_boot_begin(ani_sketch *sk, float minIdentity, int32_t minFragments, int32_t replicates, uint32_t seed)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  if (replicates < 1 || replicates > kCiMaxReplicates) return fail(ANI_ERR_ARG, "%d replicates: 1 to %d are taken", replicates, kCiMaxReplicates);
  memcpy(&sk->bootMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->bootMinIdBits = 0;                  // -0.0 counts as 0
  sk->bootMinFragments = (uint32_t)minFragments;
  sk->bootReplicates = (uint32_t)replicates; sk->bootSeed = seed;
  sk->bootPending.clear(); sk->ctx->bootStage.clear();
  sk->boot = true;
  return ANI_OK;
}

int ani_sketch_boot_take(ani_sketch *sk, ani_boot_t **rec, uint64_t **sums, size_t *n)
{
  if (!sk || !rec || !n) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->boot) return fail(ANI_ERR_ARG, "ani_sketch_boot_take without ani_sketch_boot_begin");
  *rec = nullptr; *n = 0;
  if (sums) *sums = nullptr;
  BootBuf &pd = sk->bootPending;
  if (pd.n == 0) { pd.clear(); return ANI_OK; }
  *rec = pd.rec; *n = pd.n;                     // the buffers themselves: ani_free releases them
  if (sums) *sums = pd.sums; else free(pd.sums);
  pd.rec = nullptr; pd.sums = nullptr; pd.n = pd.cap = 0;
  return ANI_OK;
}

int ani_sketch_boot_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->boot) return fail(ANI_ERR_ARG, "ani_sketch_boot_end without ani_sketch_boot_begin");
  sk->bootPending.clear(); sk->ctx->bootStage.clear();
  sk->boot = false;
  return ANI_OK;
}

// ---- the best reference of every query fragment (ani_abi.h: ani_sketch_paint_begin) ----
int ani_sketch_paint_begin(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (sk->paint) return fail(ANI_ERR_ARG, "ani_sketch_paint_begin while the mode is on");
  sk->paintPending.clear(); sk->ctx->paintStage.clear();
  sk->paint = true;
  return ANI_OK;
}

int ani_sketch_paint_take(ani_sketch *sk, ani_paint_t **rec, size_t *n)
{
  if (!sk || !rec || !n) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->paint) return fail(ANI_ERR_ARG, "ani_sketch_paint_take without ani_sketch_paint_begin");
  *rec = nullptr; *n = 0;
  PaintBuf &pd = sk->paintPending;
  if (pd.n == 0) { pd.clear(); return ANI_OK; }
  *rec = pd.rec; *n = pd.n;                     // the buffer itself: ani_free releases it
  pd.rec = nullptr; pd.n = pd.cap = 0;
  return ANI_OK;
}

int ani_sketch_paint_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->paint) return fail(ANI_ERR_ARG, "ani_sketch_paint_end without ani_sketch_paint_begin");
  ani_ctx *ctx = sk->ctx;
  HIP_TRY(hipSetDevice(sk->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  sk->paintPending.clear(); ctx->paintStage.clear();
  for (DevBuf *b : {&ctx->paintBest, &ctx->paintSecond, &ctx->paintGenomes, &ctx->paintWin, &ctx->paintFlags, &ctx->paintOff, &ctx->paintRec}) b->release();
  sk->paint = false;
  return ANI_OK;
}

// ---- collinear blocks of the best hits (ani_abi.h: ani_sketch_synteny_begin) ----
int ani_sketch_synteny_begin(ani_sketch *sk, float minIdentity, int32_t minFragments)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!(minIdentity >= 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside [0, 100]", (double)minIdentity);
  if (minFragments < 1) return fail(ANI_ERR_ARG, "minFragments %d below 1", minFragments);
  memcpy(&sk->synMinIdBits, &minIdentity, 4);
  if (minIdentity == 0.0f) sk->synMinIdBits = 0;                   // -0.0 counts as 0
  sk->synMinFragments = (uint32_t)minFragments;
  sk->synPending.clear(); sk->ctx->synStage.clear();
  sk->synteny = true;
  return ANI_OK;
}

int ani_sketch_synteny_take(ani_sketch *sk, ani_synteny_t **pairs, size_t *nPairs, ani_synblock_t **blocks, size_t *nBlocks)
{
  if (!sk || !pairs || !nPairs || !blocks || !nBlocks) return fail(ANI_ERR_ARG, "null argument");
  if (!sk->synteny) return fail(ANI_ERR_ARG, "ani_sketch_synteny_take without ani_sketch_synteny_begin");
  *pairs = nullptr; *nPairs = 0; *blocks = nullptr; *nBlocks = 0;
  SynBufs &pd = sk->synPending;
  if (pd.pairs.n == 0) { pd.clear(); return ANI_OK; }
  *pairs = pd.pairs.rec; *nPairs = pd.pairs.n;  // the buffers themselves: ani_free releases them
  pd.pairs.rec = nullptr; pd.pairs.n = pd.pairs.cap = 0;
  if (pd.blocks.n == 0) { pd.blocks.clear(); return ANI_OK; }
  *blocks = pd.blocks.rec; *nBlocks = pd.blocks.n;
  pd.blocks.rec = nullptr; pd.blocks.n = pd.blocks.cap = 0;
  return ANI_OK;
}

int ani_sketch_synteny_end(ani_sketch *sk)
{
  if (!sk) return fail(ANI_ERR_ARG, "null sketch");
  if (!sk->synteny) return fail(ANI_ERR_ARG, "ani_sketch_synteny_end without ani_sketch_synteny_begin");
  sk->synPending.clear(); sk->ctx->synStage.clear();
  sk->synteny = false;
  return ANI_OK;
}

// rule 6: a pure host function
int ani_paint_merge(const ani_paint_t *a, size_t na, const ani_paint_t *b, size_t nb, ani_paint_t **out, size_t *n)
{
  if (!out || !n || (na && !a) || (nb && !b)) return fail(ANI_ERR_ARG, "null argument");
  *out = nullptr; *n = 0;
  auto before = [](const ani_paint_t &x, const ani_paint_t &y) {
    return x.qryGenomeId < y.qryGenomeId || (x.qryGenomeId == y.qryGenomeId && x.querySeqId < y.querySeqId); };
  for (size_t i = 1; i < na; i++) if (!before(a[i - 1], a[i])) return fail(ANI_ERR_ARG, "ani_paint_merge: the first list is not in (qryGenomeId, querySeqId) order at %zu", i);
  for (size_t i = 1; i < nb; i++) if (!before(b[i - 1], b[i])) return fail(ANI_ERR_ARG, "ani_paint_merge: the second list is not in (qryGenomeId, querySeqId) order at %zu", i);
  if (na + nb == 0) return ANI_OK;
  if (na + nb > SIZE_MAX / sizeof(ani_paint_t)) return fail(ANI_ERR_NOMEM, "host allocation of paint records failed");
  ani_paint_t *o = (ani_paint_t *)malloc((na + nb) * sizeof(ani_paint_t));
  if (!o) return fail(ANI_ERR_NOMEM, "host allocation of %zu paint records failed", na + nb);
  // rule 2 on (identity bits, genome id): does (xb, xg) come before (yb, yg)?
  auto first = [](uint32_t xb, int32_t xg, uint32_t yb, int32_t yg) { return xb > yb || (xb == yb && xg < yg); };
  auto idb = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
  size_t i = 0, j = 0, m = 0;
  while (i < na || j < nb) {
    if (j >= nb || (i < na && before(a[i], b[j]))) { o[m++] = a[i++]; continue; }
    if (i >= na || before(b[j], a[i])) { o[m++] = b[j++]; continue; }
    const ani_paint_t &x = a[i++], &y = b[j++];
    const bool xFirst = first(idb(x.identity), x.refGenomeId, idb(y.identity), y.refGenomeId);
    const ani_paint_t &w = xFirst ? x : y, &l = xFirst ? y : x;      // the winner's record and the other's
    ani_paint_t r = w;
    r.genomes = x.genomes + y.genomes; r.reserved = 0;
    // the second: the loser's first, or the winner's own second
    r.secondGenomeId = l.refGenomeId; r.secondIdentity = l.identity;
    if (w.secondGenomeId >= 0 && first(idb(w.secondIdentity), w.secondGenomeId, idb(l.identity), l.refGenomeId)) {
      r.secondGenomeId = w.secondGenomeId; r.secondIdentity = w.secondIdentity; }
    o[m++] = r;
  }
  *out = o; *n = m;
  return ANI_OK;
}

}  // extern "C"

// tests/emu/Makefile compiles every unit on its own and says so with ANI_EMU_UNITS_SPLIT.  A tests/ directory from before
// engine_graph.hip and engine_sig.hip existed (an older suite run over this tree) lists neither and defines nothing: for that Makefile
// alone the two units that came out of this one are compiled with it.  hipcc never takes this branch (build_lib.sh).
#if defined(ANI_HIP_EMU) && !defined(ANI_EMU_UNITS_SPLIT)
#include "engine_graph.hip"
#include "engine_sig.hip"
#endif
