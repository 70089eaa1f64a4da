// engine_graph.hip — what works on finished ANI rows: their greedy clustering (ani_cluster_greedy, kernels/cluster.hpp) and their trees:
// average linkage (ani_tree_average, kernels/tree.hpp), neighbour joining (ani_tree_nj, kernels/nj.hpp) and single linkage with its
// minimum spanning tree (ani_tree_single, kernels/single.hpp), whose pieces ani_tree_single_sketch (engine_sig.hip) calls too.
#include "host/engine.hpp"
#include "kernels/cluster.hpp"
#include "kernels/tree.hpp"
#include "kernels/nj.hpp"
#include "kernels/single.hpp"

namespace anih {
using namespace ani;

// ---- greedy clustering of the pair graph (ani_cluster_greedy) ----
// Device memory per row: 20 (rows) + 2 x 12 (keys and positions) + 12 (the sort's ping-pong) bytes at the peak, the 12-byte edge list
// after the sort's inputs are gone; per edge end 8 (CSR); per genome 40.  Every buffer is the pool's and goes back to it on return.
int cluster_greedy(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, float minIdentity, int32_t *representative, float *identityToRep)
{
  for (int32_t i = 0; i < nG; i++) { representative[i] = i; identityToRep[i] = 0.0f; }
  if (n == 0) return ANI_OK;
  // every buffer goes back to the pool on return (the launches below take plain pointers, never the holder)
  enum { ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, E_LO, E_HI, E_W, LOW, HIGH, DEG, FILL, OFF, NBR, NBR_W, STATE, REP, REP_W, FLAGS, SORT, NBUF };
  struct Bufs { DevBuf b[NBUF]; Bufs() = default; Bufs(const Bufs &) = delete; ~Bufs() { for (DevBuf &x : b) x.release(); } } B;
  auto buf = [&](int i, size_t bytes, void **out) { const int rc = B.b[i].ensure(bytes); *out = B.b[i].p; return rc; };
  hipStream_t st = ctx->stream;
  int b = 1;
  while (b < 31 && ((uint32_t)(nG - 1) >> b) != 0) b++;          // bit width of the largest id
  const size_t V = (size_t)nG;
  ani_cgi_t *dRows; uint64_t *keysA, *keysB; uint32_t *valsA, *valsB, *flags, *off, *state; int32_t *lowDeg, *highDeg, *deg, *fill, *rep; float *repW;
  TRY(buf(ROWS, n * sizeof(ani_cgi_t), (void **)&dRows)); TRY(buf(KEYS_A, n * 8, (void **)&keysA)); TRY(buf(KEYS_B, n * 8, (void **)&keysB));
  TRY(buf(VALS_A, n * 4, (void **)&valsA)); TRY(buf(VALS_B, n * 4, (void **)&valsB)); TRY(buf(FLAGS, 64, (void **)&flags));
  TRY(buf(LOW, V * 4, (void **)&lowDeg)); TRY(buf(HIGH, V * 4, (void **)&highDeg)); TRY(buf(DEG, V * 4, (void **)&deg));
  TRY(buf(FILL, V * 8, (void **)&fill)); TRY(buf(OFF, V * 4 + 4, (void **)&off)); TRY(buf(STATE, V * 4, (void **)&state));
  TRY(buf(REP, V * 4, (void **)&rep)); TRY(buf(REP_W, V * 4, (void **)&repW));
  // flags: [0] a bad id, [1] the edge count, [2..3] the undecided counters of the rounds
  uint32_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));

  // one upload; keys; the stable sort puts the rows of a pair next to each other in the order given
  HIP_TRY(hipMemcpyAsync(dRows, rows, n * sizeof(ani_cgi_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(flags, 0, 64, st));
  HIP_TRY(hipMemsetAsync(lowDeg, 0, V * 4, st)); HIP_TRY(hipMemsetAsync(highDeg, 0, V * 4, st));
  hipLaunchKernelGGL(k_cluster_keys, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, nG, b, keysA, valsA, flags);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, flags, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (host[0]) return fail(ANI_ERR_ARG, "a row names a genome outside [0, %d)", nG);
  size_t tb = 0;
  int rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, nullptr, &tb, st);
  void *sortTmp = nullptr;
  if (rc == 0) { TRY(buf(SORT, tb + 256, &sortTmp)); rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, sortTmp, &tb, st); }
  if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the pair keys failed (%d)", rc);
  B.b[SORT].release(); B.b[KEYS_A].release(); B.b[VALS_A].release();

  // fold + threshold -> edge list (at most one edge per sorted row) and the degrees
  int32_t *eLo, *eHi; float *eW;
  TRY(buf(E_LO, n * 4, (void **)&eLo)); TRY(buf(E_HI, n * 4, (void **)&eHi)); TRY(buf(E_W, n * 4, (void **)&eW));
  hipLaunchKernelGGL(k_cluster_fold, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (const uint32_t *)valsB, (const ani_cgi_t *)dRows,
                     (uint64_t)n, b, minIdentity, flags + 1, eLo, eHi, eW, lowDeg, highDeg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, flags + 1, 4, hipMemcpyDeviceToHost, st));
  hipLaunchKernelGGL(k_cluster_degrees, dim3(grid_for(V)), dim3(256), 0, st, nG, (const int32_t *)lowDeg, (const int32_t *)highDeg, deg, fill);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t nE = host[0];
  if (nE == 0) return ANI_OK;                          // no edge: every genome is its own representative
  B.b[ROWS].release(); B.b[KEYS_B].release(); B.b[VALS_B].release();

  // CSR over both directions: offsets = prefix sum of the degrees (device_scan: ANI_ERR_LIMIT beyond 2^32 - 16 entries)
  uint64_t total = 0;
  TRY(device_scan(ctx, deg, off, (uint32_t)V, &total));
  const uint32_t tot32 = (uint32_t)total;
  HIP_TRY(hipMemcpyAsync(off + V, &tot32, 4, hipMemcpyHostToDevice, st));
  int32_t *nbr; float *nbrW;
  TRY(buf(NBR, (size_t)total * 4, (void **)&nbr)); TRY(buf(NBR_W, (size_t)total * 4, (void **)&nbrW));
  hipLaunchKernelGGL(k_cluster_scatter, dim3(grid_for(nE)), dim3(256), 0, st, nE, (const int32_t *)eLo, (const int32_t *)eHi, (const float *)eW,
                     (const uint32_t *)off, (const int32_t *)lowDeg, fill, nbr, nbrW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(state, 0, V * 4, st));

  // greedy rounds: batches of kRounds launches; the last launch of a batch counts the undecided vertices, the count is copied back
  // asynchronously and read while the next batch runs (a batch after the last one with work only finds decided vertices)
  constexpr int kRounds = 8;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
  if (hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ev[0]); return fail(ANI_ERR_DEVICE, "hipEventCreate failed"); }
  struct EvGuard { hipEvent_t *e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } evGuard{ev};
  const unsigned grid = grid_for(V, kTPB);
  // every launch decides at least the lowest undecided vertex (its lower neighbours were all decided before the launch started)
  const uint64_t maxBatches = V / kRounds + 3;
  bool done = false;
  for (uint64_t batch = 0; !done; batch++) {
    if (batch > maxBatches) return fail(ANI_ERR_INTERNAL, "greedy rounds did not converge after %llu launches", (unsigned long long)(batch * kRounds));
    const int slot = (int)(batch & 1);
    uint32_t *und = flags + 2 + slot;
    HIP_TRY(hipMemsetAsync(und, 0, 4, st));
    for (int r = 0; r < kRounds; r++) {
      uint32_t *count = r == kRounds - 1 ? und : nullptr;
      hipLaunchKernelGGL(k_cluster_round, dim3(grid), dim3(kTPB), 0, st, nG, (const uint32_t *)off, (const int32_t *)lowDeg, (const int32_t *)nbr, state, count);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host + 2 + slot, und, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev[slot], st));
    if (batch > 0) { HIP_TRY(hipEventSynchronize(ev[slot ^ 1])); done = host[2 + (slot ^ 1)] == 0; }
  }
  hipLaunchKernelGGL(k_cluster_assign, dim3(grid), dim3(kTPB), 0, st, nG, (const uint32_t *)off, (const int32_t *)nbr, (const float *)nbrW,
                     (const uint32_t *)state, rep, repW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(representative, rep, V * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(identityToRep, repW, V * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ANI_OK;
}

// ---- average-linkage (UPGMA) tree of the pair values (ani_tree_average) ----
// Device memory: 4 bytes per matrix cell (n x ld, ld = n rounded up to 64) plus 40 per genome; per row 20 + 2 x 12 + 12 bytes while the
// pairs are folded, all of it released before the merges.  The merges are a plain enqueue loop, one k_tree_merge per merge, each
// reading its pair from device memory; the result is copied back once at the end.  Every buffer is the pool's and goes back on return.
int tree_average(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, float missingIdentity, int32_t *children, float *height)
{
  enum { ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, FLAGS, SORT, DMAT, ROWMIN, STATE, PART, OUT, NBUF };
  struct Bufs { DevBuf b[NBUF]; Bufs() = default; Bufs(const Bufs &) = delete; ~Bufs() { for (DevBuf &x : b) x.release(); } } B;
  auto buf = [&](int i, size_t bytes, void **out) { const int rc = B.b[i].ensure(bytes); *out = B.b[i].p; return rc; };
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG, M = V - 1;
  const uint64_t ld = ((uint64_t)nG + 63) & ~63ull;
  const unsigned G = grid_for(V, kTreeRows);
  const float dMissing = (float)(1.0 - (double)missingIdentity / 100.0);
  TreeArgs t;
  uint32_t *flags, *state;
  TRY(buf(DMAT, (size_t)ld * V * 4, (void **)&t.D));
  TRY(buf(FLAGS, 64, (void **)&flags)); TRY(buf(ROWMIN, V * 8, (void **)&t.rowMin)); TRY(buf(STATE, V * 12 + 16, (void **)&state));
  TRY(buf(PART, (size_t)G * 16, (void **)&t.part)); TRY(buf(OUT, M * 12, (void **)&t.children));
  t.ld = ld; t.n = nG;
  t.size = (int32_t *)state; t.id = (int32_t *)state + V; t.active = state + 2 * V; t.pick = (int32_t *)state + 3 * V;
  t.arrived = flags + 1; t.height = (float *)(t.children + 2 * M);
  // flags: [0] a bad id (1) or identity (2), [1] the arrival counter of k_tree_merge
  uint32_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));
  HIP_TRY(hipMemsetAsync(flags, 0, 64, st));
  hipLaunchKernelGGL(k_tree_fill, dim3(nG), dim3(kTPB), 0, st, t.D, ld, nG, dMissing);
  HIP_TRY(hipGetLastError());

  if (n) {
    // the pair values: keys and the stable sort as for the clustering, then one fold per pair into D
    int b = 1;
    while (b < 31 && ((uint32_t)(nG - 1) >> b) != 0) b++;          // bit width of the largest id
    ani_cgi_t *dRows; uint64_t *keysA, *keysB; uint32_t *valsA, *valsB;
    TRY(buf(ROWS, n * sizeof(ani_cgi_t), (void **)&dRows)); TRY(buf(KEYS_A, n * 8, (void **)&keysA)); TRY(buf(KEYS_B, n * 8, (void **)&keysB));
    TRY(buf(VALS_A, n * 4, (void **)&valsA)); TRY(buf(VALS_B, n * 4, (void **)&valsB));
    HIP_TRY(hipMemcpyAsync(dRows, rows, n * sizeof(ani_cgi_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tree_check, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, flags);
    hipLaunchKernelGGL(k_cluster_keys, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, nG, b, keysA, valsA, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, flags, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (host[0] & 1u) return fail(ANI_ERR_ARG, "a row names a genome outside [0, %d)", nG);
    if (host[0] & 2u) return fail(ANI_ERR_ARG, "a row has an identity outside (0, 100]");
    size_t tb = 0;
    int rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, nullptr, &tb, st);
    void *sortTmp = nullptr;
    if (rc == 0) { TRY(buf(SORT, tb + 256, &sortTmp)); rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, sortTmp, &tb, st); }
    if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the pair keys failed (%d)", rc);
    hipLaunchKernelGGL(k_tree_fold, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (const uint32_t *)valsB, (const ani_cgi_t *)dRows,
                       (uint64_t)n, b, t.D, ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int i : {ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, SORT}) B.b[i].release();
  }

  // row minima, the first pick, then one launch per merge (the last one picks nothing)
  hipLaunchKernelGGL(k_tree_rowmin, dim3(nG), dim3(kTPB), 0, st, t);
  hipLaunchKernelGGL(k_tree_first, dim3(1), dim3(kTPB), 0, st, t);
  HIP_TRY(hipGetLastError());
  for (int32_t s = 0; s + 1 < nG; s++) hipLaunchKernelGGL(k_tree_merge, dim3(G), dim3(kTPB), 0, st, t, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(children, t.children, M * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(height, t.height, M * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ANI_OK;
}

// ---- neighbour-joining tree of the pair values (ani_tree_nj) ----
// Device memory: 4 bytes per cell of the int32 matrix (n x ld, ld = n rounded up to 64) plus, beyond 64 genomes, the matrix the first
// compaction writes (7/8 n on a side: 0.77 of the first); 40 bytes per genome; per row 20 + 2 x 12 + 12 bytes while the pairs are
// folded, released before the joins.  The joins are a plain enqueue loop: per record one k_nj_scan, per join one k_nj_update, and
// whenever an eighth of the matrix's positions is retired (the host knows when: one per join) a k_nj_map / k_nj_compact pair into
// the other matrix.  Nothing is read back before the end.
int tree_nj(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, float missingIdentity, int32_t *children, float *length)
{
  enum { ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, FLAGS, SORT, QMAT_A, QMAT_B, STATE_A, STATE_B, NEWPOS, PART, OUT, NBUF };
  struct Bufs { DevBuf b[NBUF]; Bufs() = default; Bufs(const Bufs &) = delete; ~Bufs() { for (DevBuf &x : b) x.release(); } } B;
  auto buf = [&](int i, size_t bytes, void **out) { const int rc = B.b[i].ensure(bytes); *out = B.b[i].p; return rc; };
  auto round64 = [](uint64_t x) { return (x + 63) & ~63ull; };
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG, M = V - 1;
  const uint64_t ld = round64(V);
  const uint64_t second = nG > 64 ? V * 7 / 8 : 0;                // positions of the first compacted matrix
  constexpr unsigned kMaxGrid = 2048;                              // workgroups of a scan: 8 per CU
  const int32_t qMissing = (int32_t)rint((100.0 - (double)missingIdentity) * 16777216.0 / 100.0);
  NjArgs t, u;                                                     // the matrix in use, the other one
  uint32_t *flags, *newPos; char *state[2];
  TRY(buf(QMAT_A, (size_t)ld * V * 4, (void **)&t.q));
  u.q = nullptr;
  if (second) TRY(buf(QMAT_B, (size_t)round64(second) * second * 4, (void **)&u.q));
  TRY(buf(FLAGS, 64, (void **)&flags)); TRY(buf(NEWPOS, ld * 4, (void **)&newPos));
  TRY(buf(STATE_A, ld * 16, (void **)&state[0])); TRY(buf(STATE_B, ld * 16, (void **)&state[1]));
  TRY(buf(PART, (size_t)kMaxGrid * 12, (void **)&t.partQ)); TRY(buf(OUT, M * 16, (void **)&t.children));
  t.ld = ld; t.n = nG; t.cur = nG;
  t.partAB = (uint32_t *)(t.partQ + kMaxGrid); t.length = (float *)(t.children + 2 * M);
  // flags: [0] a bad id (1) or identity (2), [1] the arrival counter of k_nj_scan, [4..6] the pick
  t.arrived = flags + 1; t.pick = (int32_t *)flags + 4;
  u = NjArgs{u.q, 0, nG, 0, nullptr, nullptr, nullptr, t.pick, t.partQ, t.partAB, t.arrived, t.children, t.length};
  auto set_state = [&](NjArgs &x, int i) { x.R = (int64_t *)state[i]; x.id = (int32_t *)(state[i] + ld * 8); x.active = (uint32_t *)(state[i] + ld * 12); };
  set_state(t, 0); set_state(u, 1);
  uint32_t *host = nullptr;
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));
  HIP_TRY(hipMemsetAsync(flags, 0, 64, st));
  hipLaunchKernelGGL(k_nj_fill, dim3(nG), dim3(kTPB), 0, st, t.q, ld, nG, qMissing);
  HIP_TRY(hipGetLastError());

  if (n) {
    // the pair values: keys and the stable sort as for the clustering, then one fold per pair into q
    int b = 1;
    while (b < 31 && ((uint32_t)(nG - 1) >> b) != 0) b++;          // bit width of the largest id
    ani_cgi_t *dRows; uint64_t *keysA, *keysB; uint32_t *valsA, *valsB;
    TRY(buf(ROWS, n * sizeof(ani_cgi_t), (void **)&dRows)); TRY(buf(KEYS_A, n * 8, (void **)&keysA)); TRY(buf(KEYS_B, n * 8, (void **)&keysB));
    TRY(buf(VALS_A, n * 4, (void **)&valsA)); TRY(buf(VALS_B, n * 4, (void **)&valsB));
    HIP_TRY(hipMemcpyAsync(dRows, rows, n * sizeof(ani_cgi_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tree_check, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, flags);
    hipLaunchKernelGGL(k_cluster_keys, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, nG, b, keysA, valsA, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, flags, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (host[0] & 1u) return fail(ANI_ERR_ARG, "a row names a genome outside [0, %d)", nG);
    if (host[0] & 2u) return fail(ANI_ERR_ARG, "a row has an identity outside (0, 100]");
    size_t tb = 0;
    int rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, nullptr, &tb, st);
    void *sortTmp = nullptr;
    if (rc == 0) { TRY(buf(SORT, tb + 256, &sortTmp)); rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, sortTmp, &tb, st); }
    if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the pair keys failed (%d)", rc);
    hipLaunchKernelGGL(k_nj_fold, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (const uint32_t *)valsB, (const ani_cgi_t *)dRows,
                       (uint64_t)n, b, t.q, ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int i : {ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, SORT}) B.b[i].release();
  }

  hipLaunchKernelGGL(k_nj_rowsum, dim3((unsigned)ld), dim3(kTPB), 0, st, t);
  HIP_TRY(hipGetLastError());
  for (int32_t s = 0; s + 1 < nG; s++) {
    const uint32_t cur = (uint32_t)t.cur, rowsPerTile = cur <= 4096 ? 16 : 64;
    const uint64_t tiles = (uint64_t)((cur + kNjCols - 1) / kNjCols) * ((cur + rowsPerTile - 1) / rowsPerTile);
    hipLaunchKernelGGL(k_nj_scan, dim3((unsigned)std::min<uint64_t>(tiles, kMaxGrid)), dim3(kTPB), 0, st, t, s, rowsPerTile);
    if (s + 2 == nG) break;                                        // the last record joins nothing
    hipLaunchKernelGGL(k_nj_update, dim3(grid_for(cur, kTPB)), dim3(kTPB), 0, st, t);
    const uint64_t m = (uint64_t)(nG - s - 1);                     // active positions now
    if (cur > 64 && 8 * m <= 7 * (uint64_t)cur) {
      u.cur = (int32_t)m; u.ld = round64(m);
      hipLaunchKernelGGL(k_nj_map, dim3(1), dim3(kTPB), 0, st, t, u, newPos);
      hipLaunchKernelGGL(k_nj_compact, dim3(cur), dim3(kTPB), 0, st, t, u, (const uint32_t *)newPos);
      std::swap(t, u);
    }
    if ((s & 255) == 255) HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(children, t.children, M * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(length, t.length, M * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ANI_OK;
}

// ---- single-linkage tree = minimum spanning forest of the pairs with rows (ani_tree_single) ----
// Device memory per row: 20 (rows) + 2 x 12 (keys and positions) + 12 (the sort's ping-pong) = 56 bytes during the first sort, then
// 20 + 12 + 4 (edge positions) per row and 20 per edge while the edges are compacted; per edge 44 during the second sort and 33 during the
// rounds; per genome 12 (component, hook, best edge) and 13 per forest edge of the result.  Nothing is proportional to nGenomes^2.
// One count is read back per round (the live edges), which also bounds the loop; every buffer is the pool's and goes back on return.
// The pieces are shared with ani_tree_single_sketch (section 2.16), which folds further edges into the forest strip by strip.
// a ranked list (host/engine.hpp: SingleEdges) as the kernels take it
static ani::SingleList single_list(const SingleEdges &e)
{
  return ani::SingleList{e.lo.as<uint32_t>(), e.hi.as<uint32_t>(), e.d.as<uint32_t>(), e.src.as<uint8_t>(), e.n};
}

// The front half: the rows are uploaded and checked, the stable sort puts the rows of a pair next to each other in the order given, and
// the pairs below d_missing come out as edges in (lo, hi) order with the input of the sort by distance.  pairKeys (may be null): the
// sorted distinct keys lo << b | hi of every non-self pair with rows, whatever its distance.
int single_front(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, uint32_t dmBits, SingleEdges *edges, DevBuf *pairKeys, uint32_t *nKeys)
{
  enum { ROWS, KEYS_A, KEYS_B, VALS_A, VALS_B, FLAGS, SORT, FLAG, POS, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const int b = id_bits(nG);
  edges->n = 0;
  if (nKeys) *nKeys = 0;
  if (!n) return ANI_OK;
  // flags: [0] a bad id (1) or identity (2)
  uint32_t *flags, *host = nullptr;
  TRY(B.get(FLAGS, 64, (void **)&flags));
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));
  HIP_TRY(hipMemsetAsync(flags, 0, 64, st));

  // the pair values: keys and the stable sort as for the clustering
  ani_cgi_t *dRows; uint64_t *keysA, *keysB; uint32_t *valsA, *valsB;
  TRY(B.get(ROWS, n * sizeof(ani_cgi_t), (void **)&dRows)); TRY(B.get(KEYS_A, n * 8, (void **)&keysA)); TRY(B.get(KEYS_B, n * 8, (void **)&keysB));
  TRY(B.get(VALS_A, n * 4, (void **)&valsA)); TRY(B.get(VALS_B, n * 4, (void **)&valsB));
  HIP_TRY(hipMemcpyAsync(dRows, rows, n * sizeof(ani_cgi_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_tree_check, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, flags);
  hipLaunchKernelGGL(k_cluster_keys, dim3(grid_for(n)), dim3(256), 0, st, (const ani_cgi_t *)dRows, (uint64_t)n, nG, b, keysA, valsA, flags);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, flags, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (host[0] & 1u) return fail(ANI_ERR_ARG, "a row names a genome outside [0, %d)", nG);
  if (host[0] & 2u) return fail(ANI_ERR_ARG, "a row has an identity outside (0, 100]");
  if (dmBits == 0) return ANI_OK;                                  // (d_missing = 0: no pair lies below it, and nothing is left to mask)
  size_t tb = 0;
  int rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, nullptr, &tb, st);
  void *sortTmp = nullptr;
  if (rc == 0) { TRY(B.get(SORT, tb + 256, &sortTmp)); rc = ani_sort_pairs_u64_u32(keysA, keysB, valsA, valsB, n, 2 * b, sortTmp, &tb, st); }
  if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the pair keys failed (%d)", rc);
  for (int i : {SORT, KEYS_A, VALS_A}) B.b[(size_t)i].release();
  int32_t *flag; uint32_t *pos;
  TRY(B.get(FLAG, n * 4, (void **)&flag)); TRY(B.get(POS, n * 4, (void **)&pos));
  if (pairKeys) {
    hipLaunchKernelGGL(k_single_keyflag, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (uint64_t)n, b, flag);
    HIP_TRY(hipGetLastError());
    uint64_t nK = 0;
    TRY(device_scan(ctx, flag, pos, (uint32_t)n, &nK));
    TRY(pairKeys->ensure(nK ? (size_t)nK * 8 : 8));
    hipLaunchKernelGGL(k_single_keys, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (uint64_t)n, (const int32_t *)flag, (const uint32_t *)pos,
                       pairKeys->as<uint64_t>());
    HIP_TRY(hipGetLastError());
    *nKeys = (uint32_t)nK;
  }
  // the edges (pairs below d_missing), compacted in (lo, hi) order
  hipLaunchKernelGGL(k_single_flag, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (const uint32_t *)valsB, (const ani_cgi_t *)dRows,
                     (uint64_t)n, b, dmBits, flag);
  HIP_TRY(hipGetLastError());
  uint64_t nE64 = 0;
  TRY(device_scan(ctx, flag, pos, (uint32_t)n, &nE64));
  B.b[FLAG].release();
  const uint32_t nE = (uint32_t)nE64;
  if (!nE) { HIP_TRY(hipStreamSynchronize(st)); return ANI_OK; }
  TRY(edges->lo.ensure((size_t)nE * 4)); TRY(edges->hi.ensure((size_t)nE * 4)); TRY(edges->dKey.ensure((size_t)nE * 8)); TRY(edges->idx.ensure((size_t)nE * 4));
  hipLaunchKernelGGL(k_single_pairs, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t *)keysB, (const uint32_t *)valsB, (const ani_cgi_t *)dRows,
                     (uint64_t)n, b, dmBits, (const uint32_t *)pos, edges->lo.as<uint32_t>(), edges->hi.as<uint32_t>(), edges->dKey.as<uint64_t>(),
                     edges->idx.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  edges->n = nE;
  return ANI_OK;
}

// Rule 3's order: a stable sort over the bits of d leaves equal distances in (lo, hi) order, so an edge's position is its rank.  Takes
// edges in (lo, hi) order (lo, hi, dKey, idx) and leaves them ranked (lo, hi, d, src), every one with the source byte given.
int single_rank(ani_ctx *ctx, SingleEdges *e, uint8_t source)
{
  if (!e->n) return ANI_OK;
  hipStream_t st = ctx->stream;
  const size_t nE = e->n;
  enum { DKEY_B, IDX_B, SORT, NBUF };
  DevBufs B(NBUF);
  uint64_t *dKeyB; uint32_t *idxB;
  TRY(B.get(DKEY_B, nE * 8, (void **)&dKeyB)); TRY(B.get(IDX_B, nE * 4, (void **)&idxB));
  size_t tb = 0;
  int rc = ani_sort_pairs_u64_u32(e->dKey.as<uint64_t>(), dKeyB, e->idx.as<uint32_t>(), idxB, nE, 32, nullptr, &tb, st);
  void *sortTmp = nullptr;
  if (rc == 0) { TRY(B.get(SORT, tb + 256, &sortTmp)); rc = ani_sort_pairs_u64_u32(e->dKey.as<uint64_t>(), dKeyB, e->idx.as<uint32_t>(), idxB, nE, 32, sortTmp, &tb, st); }
  if (rc != 0) return fail(ANI_ERR_DEVICE, "radix sort of the pair distances failed (%d)", rc);
  B.b[SORT].release(); e->dKey.release(); e->idx.release();
  SingleEdges r;
  TRY(r.lo.ensure(nE * 4)); TRY(r.hi.ensure(nE * 4)); TRY(r.d.ensure(nE * 4)); TRY(r.src.ensure(nE));
  const ani::SingleList out = single_list(r);                            // (the launches take plain pointers, never the holder)
  hipLaunchKernelGGL(k_single_rank, dim3(grid_for(nE)), dim3(256), 0, st, (uint32_t)nE, (const uint32_t *)idxB, (const uint32_t *)e->lo.as<uint32_t>(),
                     (const uint32_t *)e->hi.as<uint32_t>(), (const uint64_t *)dKeyB, source, (uint32_t *)out.lo, (uint32_t *)out.hi, (uint32_t *)out.d,
                     (uint8_t *)out.src);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  r.n = (uint32_t)nE;
  e->swap(r);
  return ANI_OK;
}

// Two ranked lists that share no edge -> one, in `x`; `y` is emptied.
int single_merge(ani_ctx *ctx, SingleEdges *x, SingleEdges *y)
{
  if (!y->n) return ANI_OK;
  if (!x->n) { x->swap(*y); y->release(); return ANI_OK; }
  const uint64_t nE = (uint64_t)x->n + y->n;
  if (nE > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%llu edges in one fold: the forest stage takes fewer than 2^32 - 16", (unsigned long long)nE);
  SingleEdges r;
  TRY(r.lo.ensure((size_t)nE * 4)); TRY(r.hi.ensure((size_t)nE * 4)); TRY(r.d.ensure((size_t)nE * 4)); TRY(r.src.ensure((size_t)nE));
  const ani::SingleList out = single_list(r);
  hipLaunchKernelGGL(k_single_merge, dim3(grid_for((size_t)nE)), dim3(256), 0, ctx->stream, single_list(*x), single_list(*y), (uint32_t *)out.lo, (uint32_t *)out.hi,
                     (uint32_t *)out.d, (uint8_t *)out.src);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  r.n = (uint32_t)nE;
  x->swap(r);
  y->release();
  return ANI_OK;
}

// The forest stage: Boruvka rounds over a ranked edge list; the chosen edges stay, in rank order (a ranked list again).  A round in
// which e edges join two components hooks every component that has one, so the components with edges at least halve: ceil(log2 V) rounds
// with live edges, and one more that finds none.  The rounds are added to ctx->treeSingleRounds.
int single_forest(ani_ctx *ctx, int32_t nG, SingleEdges *e)
{
  if (!e->n) return ANI_OK;
  enum { FLAGS, CHOSEN, LIVE_A, LIVE_B, COMP, PAR, BEST, POS, NBUF };
  DevBufs B(NBUF);
  hipStream_t st = ctx->stream;
  const size_t V = (size_t)nG;
  const uint32_t nE = e->n;
  const int b = id_bits(nG);
  // flags: [1] the live edges of a round, [2] a hook path that did not end
  uint32_t *flags, *host = nullptr;
  TRY(B.get(FLAGS, 64, (void **)&flags));
  TRY(pinned_buffer(ctx, 1, 64, (void **)&host));
  HIP_TRY(hipMemsetAsync(flags, 0, 64, st));
  const uint32_t *uLo = e->lo.as<uint32_t>(), *uHi = e->hi.as<uint32_t>();
  uint32_t *live[2], *comp, *par, *best; int32_t *chosen;
  TRY(B.get(CHOSEN, (size_t)nE * 4, (void **)&chosen));
  TRY(B.get(LIVE_A, (size_t)nE * 4, (void **)&live[0])); TRY(B.get(LIVE_B, (size_t)nE * 4, (void **)&live[1]));
  TRY(B.get(COMP, V * 4, (void **)&comp)); TRY(B.get(PAR, V * 4, (void **)&par)); TRY(B.get(BEST, V * 4, (void **)&best));
  HIP_TRY(hipMemsetAsync(chosen, 0, (size_t)nE * 4, st));
  const unsigned gridV = grid_for(V);
  hipLaunchKernelGGL(k_single_init, dim3(gridV), dim3(256), 0, st, (uint32_t)V, comp, best);
  HIP_TRY(hipGetLastError());
  const int maxRounds = b + 3;
  const uint32_t *liveIn = nullptr; uint32_t nLive = nE;
  for (int round = 0; nLive; round++) {
    if (round >= maxRounds) return fail(ANI_ERR_INTERNAL, "the spanning forest did not converge after %d rounds", round);
    uint32_t *liveOut = live[round & 1];
    HIP_TRY(hipMemsetAsync(flags + 1, 0, 4, st));
    hipLaunchKernelGGL(k_single_best, dim3(grid_for(nLive)), dim3(256), 0, st, liveIn, nLive, uLo, uHi, (const uint32_t *)comp, best, liveOut, flags + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, flags + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (host[1]) return fail(ANI_ERR_INTERNAL, "the hooks of round %d hold a cycle", round - 1);
    if (host[0] > nLive) return fail(ANI_ERR_INTERNAL, "the live edges grew from %u to %u", nLive, host[0]);
    ctx->treeSingleRounds++;
    liveIn = liveOut; nLive = host[0];
    if (!nLive) break;
    hipLaunchKernelGGL(k_single_hook, dim3(gridV), dim3(256), 0, st, (uint32_t)V, (const uint32_t *)comp, (const uint32_t *)best, uLo, uHi, par, chosen);
    hipLaunchKernelGGL(k_single_jump, dim3(gridV), dim3(256), 0, st, (uint32_t)V, (const uint32_t *)comp, par, flags + 2);
    hipLaunchKernelGGL(k_single_label, dim3(gridV), dim3(256), 0, st, (uint32_t)V, comp, (const uint32_t *)par, best);
    HIP_TRY(hipGetLastError());
  }
  for (int i : {LIVE_A, LIVE_B, COMP, PAR, BEST}) B.b[(size_t)i].release();

  // the chosen edges, compacted in rank order
  uint32_t *cpos;
  TRY(B.get(POS, (size_t)nE * 4, (void **)&cpos));
  uint64_t nRec = 0;
  TRY(device_scan(ctx, chosen, cpos, nE, &nRec));
  if (nRec > V - 1) return fail(ANI_ERR_INTERNAL, "%llu forest edges over %d genomes", (unsigned long long)nRec, nG);
  SingleEdges f;
  if (nRec) {
    TRY(f.lo.ensure((size_t)nRec * 4)); TRY(f.hi.ensure((size_t)nRec * 4)); TRY(f.d.ensure((size_t)nRec * 4)); TRY(f.src.ensure((size_t)nRec));
    const ani::SingleList out = single_list(f);
    hipLaunchKernelGGL(k_single_records, dim3(grid_for(nE)), dim3(256), 0, st, nE, (const int32_t *)chosen, (const uint32_t *)cpos, uLo, uHi,
                       (const uint32_t *)e->d.as<uint32_t>(), (const uint8_t *)e->src.as<uint8_t>(), (uint32_t *)out.lo, (uint32_t *)out.hi, (uint32_t *)out.d,
                       (uint8_t *)out.src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    f.n = (uint32_t)nRec;
  }
  e->swap(f);
  return ANI_OK;
}

// The linkage: the forest edges (brought back from the device) in rank order through a union-find, then rule 5's joins to leaf 0 (a
// cluster not yet joined when its smallest leaf k comes up: every smaller leaf is with leaf 0 by then).  source (may be null): per merge
// the forest edge's source byte, 2 for a join to leaf 0.
int single_finish(ani_ctx *ctx, const SingleEdges &forest, int32_t nG, float dMissing, int32_t *children, float *height, int32_t *edges, uint8_t *source)
{
  const size_t V = (size_t)nG, M = V - 1, nF = forest.n;
  std::vector<uint32_t> lo(nF), hi(nF), dist(nF); std::vector<uint8_t> src(nF);
  if (nF) {
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(lo.data(), forest.lo.p, nF * 4, hipMemcpyDeviceToHost, st)); HIP_TRY(hipMemcpyAsync(hi.data(), forest.hi.p, nF * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dist.data(), forest.d.p, nF * 4, hipMemcpyDeviceToHost, st)); HIP_TRY(hipMemcpyAsync(src.data(), forest.src.p, nF, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  std::vector<int32_t> up(V), id(V);
  for (size_t i = 0; i < V; i++) { up[i] = (int32_t)i; id[i] = (int32_t)i; }
  auto find = [&](int32_t x) { while (up[(size_t)x] != x) { up[(size_t)x] = up[(size_t)up[(size_t)x]]; x = up[(size_t)x]; } return x; };
  size_t s = 0;
  auto merge = [&](int32_t a, int32_t c, float d, uint8_t from) {
    const int32_t ra = find(a), rb = find(c);
    if (ra == rb) return false;
    const int32_t ia = id[(size_t)ra], ib = id[(size_t)rb];
    children[2 * s] = ia < ib ? ia : ib; children[2 * s + 1] = ia < ib ? ib : ia;
    height[s] = d;
    if (edges) { edges[2 * s] = a; edges[2 * s + 1] = c; }
    if (source) source[s] = from;
    up[(size_t)rb] = ra; id[(size_t)ra] = (int32_t)(V + s);
    s++;
    return true;
  };
  for (size_t r = 0; r < nF; r++) {
    float d; memcpy(&d, &dist[r], 4);
    if (lo[r] >= V || hi[r] >= V || !merge((int32_t)lo[r], (int32_t)hi[r], d, src[r])) return fail(ANI_ERR_INTERNAL, "the forest edges hold a cycle");
  }
  for (size_t k = 1; k < V; k++) (void)merge(0, (int32_t)k, dMissing, 2);
  if (s != M) return fail(ANI_ERR_INTERNAL, "%zu merges over %d genomes", s, nG);
  return ANI_OK;
}

int tree_single(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nG, float missingIdentity, int32_t *children, float *height, int32_t *edges)
{
  const float dMissing = (float)(1.0 - (double)missingIdentity / 100.0);
  uint32_t dmBits; memcpy(&dmBits, &dMissing, 4);
  ctx->treeSingleRounds = 0;
  SingleEdges e;
  TRY(single_front(ctx, rows, n, nG, dmBits, &e, nullptr, nullptr));
  TRY(single_rank(ctx, &e, 0));
  TRY(single_forest(ctx, nG, &e));
  return single_finish(ctx, e, nG, dMissing, children, height, edges, nullptr);
}

}  // namespace anih

extern "C" {

int ani_cluster_greedy(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float minIdentity, int32_t *representative, float *identityToRep)
{
  if (!ctx || (n && !rows) || (nGenomes > 0 && (!representative || !identityToRep))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  if (!(minIdentity > 0.0f && minIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "minIdentity %g outside (0, 100]", (double)minIdentity);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  HIP_TRY(hipSetDevice(ctx->device));
  return cluster_greedy(ctx, rows, n, nGenomes, minIdentity, representative, identityToRep);
}

int ani_tree_average(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity, int32_t *children, float *height)
{
  if (!ctx || (n && !rows) || (nGenomes > 1 && (!children || !height))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  if (!(missingIdentity >= 0.0f && missingIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "missingIdentity %g outside [0, 100]", (double)missingIdentity);
  if (nGenomes > 65536) return fail(ANI_ERR_LIMIT, "%d genomes: the tree takes at most 65536", nGenomes);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  if (nGenomes <= 1) return ANI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return tree_average(ctx, rows, n, nGenomes, missingIdentity, children, height);
}

int ani_tree_nj(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity, int32_t *children, float *length)
{
  if (!ctx || (n && !rows) || (nGenomes > 1 && (!children || !length))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  if (!(missingIdentity >= 0.0f && missingIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "missingIdentity %g outside [0, 100]", (double)missingIdentity);
  if (nGenomes > 65536) return fail(ANI_ERR_LIMIT, "%d genomes: the tree takes at most 65536", nGenomes);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  if (nGenomes <= 1) return ANI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return tree_nj(ctx, rows, n, nGenomes, missingIdentity, children, length);
}

int ani_tree_single(ani_ctx *ctx, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity, int32_t *children, float *height,
                    int32_t *edges)
{
  if (!ctx || (n && !rows) || (nGenomes > 1 && (!children || !height))) return fail(ANI_ERR_ARG, "null argument");
  if (nGenomes < 0) return fail(ANI_ERR_ARG, "negative genome count");
  if (!(missingIdentity >= 0.0f && missingIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "missingIdentity %g outside [0, 100]", (double)missingIdentity);
  if (nGenomes > (1 << 30)) return fail(ANI_ERR_LIMIT, "%d genomes: the cluster ids of the tree take at most 2^30", nGenomes);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  if (nGenomes <= 1) return ANI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  try { return tree_single(ctx, rows, n, nGenomes, missingIdentity, children, height, edges); }
  catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

int ani_tree_single_rounds(const ani_ctx *ctx) { return ctx ? ctx->treeSingleRounds : 0; }

// ---- clade support (ani_abi.h: ani_tree_support) ----
namespace {

struct LeafSet { int32_t mn, mx, size; };              // of positions in the main tree's traversal order
inline LeafSet join(const LeafSet &a, const LeafSet &b)
{
  if (!a.size) return b;
  if (!b.size) return a;
  return LeafSet{std::min(a.mn, b.mn), std::max(a.mx, b.mx), a.size + b.size};
}

// rule 5: record s names two ids below nGenomes + s, and no id twice.  n - 1 such records over n leaves are one tree, rooted at the last.
bool is_tree(const int32_t *ch, int32_t n, std::vector<uint8_t> &used)
{
  used.assign((size_t)2 * n - 1, 0);
  for (int32_t s = 0; s < n - 1; s++)
    for (int k = 0; k < 2; k++) {
      const int32_t v = ch[2 * (size_t)s + k];
      if (v < 0 || v >= n + s || used[(size_t)v]) return false;
      used[(size_t)v] = 1;
    }
  return true;
}

}  // namespace

int ani_tree_support(const int32_t *children, int32_t nGenomes, const int32_t *repChildren, int32_t nReplicates, int32_t unrooted, uint32_t *support)
{
  if (nGenomes < 0 || nReplicates < 0) return fail(ANI_ERR_ARG, "negative count");
  if (nGenomes <= 1) return ANI_OK;
  if (!children || !support || (nReplicates && !repChildren)) return fail(ANI_ERR_ARG, "null argument");
  try {
    const int32_t n = nGenomes, M = n - 1;
    const size_t nodes = (size_t)2 * n - 1;
    std::vector<uint8_t> used;
    if (!is_tree(children, n, used)) return fail(ANI_ERR_ARG, "ani_tree_support: the main record list is not a tree");
    for (int32_t r = 0; r < nReplicates; r++)
      if (!is_tree(repChildren + (size_t)r * 2 * M, n, used)) return fail(ANI_ERR_ARG, "ani_tree_support: the record list of replicate %d is not a tree", r);
    // the main tree: sizes in record order, then positions from the root down (a parent's record comes after its children's): the leaves
    // of a node are the positions start .. start + size - 1
    std::vector<int32_t> size(nodes, 1), start(nodes, 0);
    for (int32_t s = 0; s < M; s++) size[(size_t)n + s] = size[(size_t)children[2 * (size_t)s]] + size[(size_t)children[2 * (size_t)s + 1]];
    for (int32_t s = M - 1; s >= 0; s--) {
      const int32_t a = children[2 * (size_t)s], b = children[2 * (size_t)s + 1];
      start[(size_t)a] = start[(size_t)n + s]; start[(size_t)b] = start[(size_t)n + s] + size[(size_t)a];
    }
    // the clades asked for as intervals (lo << 32 | hi), sorted; unrooted: the side of the split without the last position, which is an
    // interval for every main node — and so must the matching side of a replicate's node be
    std::vector<uint64_t> key; key.reserve((size_t)M);
    std::vector<uint64_t> want((size_t)M, ~0ull);        // per record; ~0: trivial
    for (int32_t s = 0; s < M; s++) {
      const int64_t lo = start[(size_t)n + s], sz = size[(size_t)n + s], hi = lo + sz - 1;
      if (!unrooted) want[(size_t)s] = ((uint64_t)lo << 32) | (uint64_t)hi;
      else if (sz >= n - 1) continue;
      else want[(size_t)s] = hi < n - 1 ? (((uint64_t)lo << 32) | (uint64_t)hi) : (uint64_t)(lo - 1);      // [0, lo - 1]
      key.push_back(want[(size_t)s]);
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    std::vector<uint32_t> count(key.size(), 0);
    std::vector<int32_t> seen(key.size(), -1);             // the last replicate that had the clade: a replicate counts once
    std::vector<LeafSet> in(nodes), out(unrooted ? nodes : 0);
    for (int32_t i = 0; i < n; i++) in[(size_t)i] = LeafSet{start[(size_t)i], start[(size_t)i], 1};
    auto look = [&](const LeafSet &x, int32_t r) {
      if (x.size < 2 || x.mx - x.mn + 1 != x.size) return;
      const uint64_t k = ((uint64_t)x.mn << 32) | (uint64_t)x.mx;
      const auto it = std::lower_bound(key.begin(), key.end(), k);
      if (it == key.end() || *it != k) return;
      const size_t at = (size_t)(it - key.begin());
      if (seen[at] != r) { seen[at] = r; count[at]++; }
    };
    for (int32_t r = 0; r < nReplicates; r++) {
      const int32_t *ch = repChildren + (size_t)r * 2 * M;
      for (int32_t s = 0; s < M; s++) {
        in[(size_t)n + s] = join(in[(size_t)ch[2 * (size_t)s]], in[(size_t)ch[2 * (size_t)s + 1]]);
        look(in[(size_t)n + s], r);
      }
      if (!unrooted) continue;
      // the other side of every node's split: the parent's other side and the sibling, from the root (whose other side is empty) down
      out[nodes - 1] = LeafSet{0, 0, 0};
      for (int32_t s = M - 1; s >= 0; s--) {
        const int32_t a = ch[2 * (size_t)s], b = ch[2 * (size_t)s + 1];
        out[(size_t)a] = join(out[(size_t)n + s], in[(size_t)b]); out[(size_t)b] = join(out[(size_t)n + s], in[(size_t)a]);
        look(out[(size_t)n + s], r);
      }
    }
    for (int32_t s = 0; s < M; s++) {
      if (want[(size_t)s] == ~0ull) { support[s] = (uint32_t)nReplicates; continue; }
      support[s] = count[(size_t)(std::lower_bound(key.begin(), key.end(), want[(size_t)s]) - key.begin())];
    }
    return ANI_OK;
  } catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

// ---- bootstrap support of a tree: the replicate trees through the method's own entry point, then ani_tree_support ----
int ani_tree_support_bootstrap(ani_ctx *ctx, int32_t method, const ani_cgi_t *rows, size_t n, int32_t nGenomes, float missingIdentity,
                               const float *repIdentity, int32_t nReplicates, const int32_t *children, uint32_t *support)
{
  if (!ctx || (n && !rows) || (nGenomes > 1 && (!children || !support)) || (n && nReplicates > 0 && !repIdentity)) return fail(ANI_ERR_ARG, "null argument");
  if (method != ANI_TREE_AVERAGE && method != ANI_TREE_NJ && method != ANI_TREE_SINGLE) return fail(ANI_ERR_ARG, "unknown tree method %d", method);
  if (nGenomes < 0 || nReplicates < 0) return fail(ANI_ERR_ARG, "negative count");
  if (!(missingIdentity >= 0.0f && missingIdentity <= 100.0f)) return fail(ANI_ERR_ARG, "missingIdentity %g outside [0, 100]", (double)missingIdentity);
  if (method == ANI_TREE_SINGLE ? nGenomes > (1 << 30) : nGenomes > 65536)
    return fail(ANI_ERR_LIMIT, "%d genomes: the tree takes at most %d", nGenomes, method == ANI_TREE_SINGLE ? 1 << 30 : 65536);
  if (n > 0xfffffff0ull) return fail(ANI_ERR_LIMIT, "%zu rows: the pair sort takes fewer than 2^32 - 16", n);
  for (size_t i = 0; i < n; i++) if (rows[i].qryGenomeId < 0 || rows[i].qryGenomeId >= nGenomes || rows[i].refGenomeId < 0 || rows[i].refGenomeId >= nGenomes)
    return fail(ANI_ERR_ARG, "row %zu: genome id outside [0, %d)", i, nGenomes);
  for (size_t i = 0; i < n * (size_t)nReplicates; i++) if (!(repIdentity[i] > 0.0f && repIdentity[i] <= 100.0f))
    return fail(ANI_ERR_ARG, "repIdentity of row %zu, replicate %zu (%g) outside (0, 100]", i / (size_t)nReplicates, i % (size_t)nReplicates, (double)repIdentity[i]);
  if (nGenomes <= 1) return ANI_OK;
  try {
    {                                                    // the main tree, as ani_tree_support will check it: before the first tree call
      std::vector<uint8_t> used;
      if (!is_tree(children, nGenomes, used)) return fail(ANI_ERR_ARG, "ani_tree_support_bootstrap: the main record list is not a tree");
    }
    const size_t M = (size_t)nGenomes - 1, B = (size_t)nReplicates;
    std::vector<ani_cgi_t> rep(rows, rows + n);
    std::vector<int32_t> repChildren(B * 2 * M);
    std::vector<float> branch(2 * M);                    // heights or lengths: not used
    for (size_t r = 0; r < B; r++) {
      for (size_t i = 0; i < n; i++) rep[i].identity = repIdentity[i * B + r];
      int32_t *ch = repChildren.data() + r * 2 * M;
      if (method == ANI_TREE_AVERAGE) TRY(ani_tree_average(ctx, rep.data(), n, nGenomes, missingIdentity, ch, branch.data()));
      else if (method == ANI_TREE_NJ) TRY(ani_tree_nj(ctx, rep.data(), n, nGenomes, missingIdentity, ch, branch.data()));
      else TRY(ani_tree_single(ctx, rep.data(), n, nGenomes, missingIdentity, ch, branch.data(), nullptr));
    }
    return ani_tree_support(children, nGenomes, repChildren.data(), nReplicates, method == ANI_TREE_NJ, support);
  } catch (const std::bad_alloc &) { return fail(ANI_ERR_NOMEM, "host allocation failed"); }
}

}  // extern "C"
