// prim_check.hip — TEST INFRASTRUCTURE: entry points that run the shared device primitives of kernels/common.hpp and the device-wide
// prefix sum (kernels/scan.hpp, anih::device_scan) on their own, so that tests/test_primitives.py can hold each of them to its
// definition (tests/prim_cases.py: numpy and Python integers).  Nothing in the product calls these; they are not part of
// include/ani_abi.h.  The check kernels call the primitives the way the product kernels do: kTPB threads, LDS arrays, the same
// template arguments.
//
// ani_prim_check(op, in, out, sizes, blocks, cap, threads, stream): workgroup b works on its own slot with its own size sizes[b].
// A slot is a number of planes of `cap` elements each (element = 4 or 8 bytes, by op): the inputs of workgroup b are the planes
// (b * IN + p) of `in`, its outputs the planes (b * OUT + p) of `out`.  A workgroup writes the elements listed below and nothing
// else, so the caller finds its filling in the rest of every plane.  n = sizes[b]; T = thread, w = wave, l = lane.
//
//   op                       elem  IN  OUT  threads      n        outputs
//   WAVE_SCAN                i32   1   2    64/128/256   -        [0][T] wave_incl_scan(in[T]), [1][T] wave_incl_scan_dpp(in[T])
//   BLOCK_EXCL_SCAN          i32   2   4    256          -        two calls in a row on one ws: [0][T] scan of in[0], [1][T] its total as
//                                                                 thread T got it, [2][T], [3][T] the same for in[1]
//   BLOCK_MAXSCAN            i32   2   2    256          -        two calls in a row on one ws: [p][T] block_incl_maxscan(in[p][T])
//   ARRAY_SCAN_LDS / _GLOBAL i32   1   2    256          <= 6144  [0][0..n) block_array_excl_scan of in[0][0..n) (in LDS / in place in `out`),
//                                                                 [1][T] the total thread T got
//   LANE_XOR_U32 / _U64      u32/u64 1 6    64/128/256   -        [m][T] lane_xor<1 << m>(in[T])
//   LANE_VALUE               i32   1   5    64/128/256   -        [j][T] lane_value(in[T], {0, 1, 31, 32, 63}[j])
//   WAVE_UNIFORM_U32 / _U64  u32/u64 1 2    256          -        x = in[w] (wave-uniform, unknown to the compiler): [0][T] wave_uniform(x);
//                                                                 [1][T] wave_uniform(x) taken with the lanes l % 4 == 1 only, ~x in the others
//   BLOCK_SORT_U32 / _U64    u32/u64 1 1    256          <= 4096  [0][0..n) block_sort of in[0..n)
//   BITONIC_U32 / _U64       u32/u64 1 1    256          <= 4096  [0][0..n) block_bitonic_sort of in[0..n) padded with ~0 to next_pow2(n)
//   WAVE_SORT_1 / _2 / _4    u64   4   4    256          <= 64 KPT [w][0..n) l1_tiny_load_sort<u64, KPT> (wave_sort_regs) of in[w][0..n), every wave its own
//   ROTL64                   u64   1   63   256          <= cap   [r - 1][i] rotl64(in[i], r), r = 1 .. 63
//   PERM_B32                 u32   2   1    256          <= cap / 4096   [0][i * 4096 + s] perm_b32(in[0][i], in[1][i], selector s): byte j of the
//                                                                 selector = bits [3 j, 3 j + 3) of s
//   ALIGNBYTE                u32   3   1    256          <= cap   [0][i] alignbyte(in[0][i], in[1][i], in[2][i])
//
// ani_prim_device_scan forwards to anih::device_scan on the context's stream.
#include "host/engine.hpp"
#include "kernels/l1.hpp"

namespace {
using namespace ani;

enum PrimOp {
  OP_WAVE_SCAN = 0, OP_BLOCK_EXCL_SCAN, OP_BLOCK_MAXSCAN, OP_ARRAY_SCAN_LDS, OP_ARRAY_SCAN_GLOBAL, OP_LANE_XOR_U32, OP_LANE_XOR_U64, OP_LANE_VALUE,
  OP_WAVE_UNIFORM_U32, OP_WAVE_UNIFORM_U64, OP_BLOCK_SORT_U32, OP_BLOCK_SORT_U64, OP_BITONIC_U32, OP_BITONIC_U64, OP_WAVE_SORT_1, OP_WAVE_SORT_2,
  OP_WAVE_SORT_4, OP_ROTL64, OP_PERM_B32, OP_ALIGNBYTE, OP_N
};
constexpr int kArrayScanCap = 3 * kTPB * 8;       // ints of LDS for ARRAY_SCAN_LDS: three passes of block_array_excl_scan
constexpr int kPermSelectors = 4096;              // four selector bytes of 0 .. 7

struct Slot {
  const void *in; void *out; const int32_t *sizes; int cap;
  template <class T> __device__ const T *src(int planes, int p) const { return (const T *)in + ((size_t)blockIdx.x * planes + p) * cap; }
  template <class T> __device__ T *dst(int planes, int p) const { return (T *)out + ((size_t)blockIdx.x * planes + p) * cap; }
  __device__ int n() const { return sizes[blockIdx.x]; }
};

__global__ __launch_bounds__(kTPB) void k_prim_wave_scan(Slot s)
{
  const int t = threadIdx.x, v = s.src<int>(1, 0)[t];
  s.dst<int>(2, 0)[t] = wave_incl_scan(v);
  s.dst<int>(2, 1)[t] = wave_incl_scan_dpp(v);
}

__global__ __launch_bounds__(kTPB) void k_prim_block_excl_scan(Slot s)
{
  __shared__ int ws[8];
  const int t = threadIdx.x;
  int tot0, tot1;
  const int r0 = block_excl_scan(s.src<int>(2, 0)[t], ws, &tot0);
  const int r1 = block_excl_scan(s.src<int>(2, 1)[t], ws, &tot1);
  s.dst<int>(4, 0)[t] = r0; s.dst<int>(4, 1)[t] = tot0;
  s.dst<int>(4, 2)[t] = r1; s.dst<int>(4, 3)[t] = tot1;
}

__global__ __launch_bounds__(kTPB) void k_prim_block_maxscan(Slot s)
{
  __shared__ int ws[8];
  const int t = threadIdx.x;
  const int r0 = block_incl_maxscan(s.src<int>(2, 0)[t], ws);
  const int r1 = block_incl_maxscan(s.src<int>(2, 1)[t], ws);
  s.dst<int>(2, 0)[t] = r0; s.dst<int>(2, 1)[t] = r1;
}

template <bool GLOBAL> __global__ __launch_bounds__(kTPB) void k_prim_array_scan(Slot s)
{
  __shared__ int lds[GLOBAL ? 1 : kArrayScanCap];
  __shared__ int ws[8];
  const int n = s.n();
  const int *in = s.src<int>(1, 0);
  int *res = s.dst<int>(2, 0);
  int *a = GLOBAL ? res : lds;
  for (int i = threadIdx.x; i < n; i += kTPB) a[i] = in[i];
  block_barrier_mem();                             // the array is complete
  const int tot = block_array_excl_scan(a, n, ws);
  if (!GLOBAL) for (int i = threadIdx.x; i < n; i += kTPB) res[i] = a[i];
  s.dst<int>(2, 1)[threadIdx.x] = tot;
}

template <class T> __global__ __launch_bounds__(kTPB) void k_prim_lane_xor(Slot s)
{
  const int t = threadIdx.x;
  const T x = s.src<T>(1, 0)[t];
  s.dst<T>(6, 0)[t] = lane_xor<1>(x);
  s.dst<T>(6, 1)[t] = lane_xor<2>(x);
  s.dst<T>(6, 2)[t] = lane_xor<4>(x);
  s.dst<T>(6, 3)[t] = lane_xor<8>(x);
  s.dst<T>(6, 4)[t] = lane_xor<16>(x);
  s.dst<T>(6, 5)[t] = lane_xor<32>(x);
}

__global__ __launch_bounds__(kTPB) void k_prim_lane_value(Slot s)
{
  const int t = threadIdx.x;
  const int32_t x = s.src<int32_t>(1, 0)[t];
  s.dst<int32_t>(5, 0)[t] = lane_value(x, 0);
  s.dst<int32_t>(5, 1)[t] = lane_value(x, 1);
  s.dst<int32_t>(5, 2)[t] = lane_value(x, 31);
  s.dst<int32_t>(5, 3)[t] = lane_value(x, 32);
  s.dst<int32_t>(5, 4)[t] = lane_value(x, 63);
}

template <class T> __global__ __launch_bounds__(kTPB) void k_prim_wave_uniform(Slot s)
{
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const T x = s.src<T>(1, 0)[t >> 6];
  s.dst<T>(2, 0)[t] = wave_uniform(x);
  T y = (T)~x;
  if ((lane & 3) == 1) y = wave_uniform(x);        // the first active lane is not lane 0
  s.dst<T>(2, 1)[t] = y;
}

template <class K, bool LDS_NETWORK> __global__ __launch_bounds__(kTPB) void k_prim_block_sort(Slot s)
{
  __shared__ K a[kBlockSortMax];
  const int n = s.n();
  const K *in = s.src<K>(1, 0);
  K *res = s.dst<K>(1, 0);
  for (int i = threadIdx.x; i < n; i += kTPB) a[i] = in[i];
  if (LDS_NETWORK) {
    const int n2 = next_pow2_dev(n);
    for (int i = n + (int)threadIdx.x; i < n2; i += kTPB) a[i] = (K)~(K)0;
    block_bitonic_sort<K>(a, n2);
  } else {
    block_sort<K>(a, n);
  }
  for (int i = threadIdx.x; i < n; i += kTPB) res[i] = a[i];
}

template <int KPT> __global__ __launch_bounds__(kTPB) void k_prim_wave_sort(Slot s)
{
  __shared__ uint64_t all[(kTPB / kWave) * kWave * KPT];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int H = s.n();
  uint64_t *hits = all + wv * kWave * KPT;          // as in k_l1_tiny: every wave its own fragment, no workgroup barrier
  const uint64_t *in = s.src<uint64_t>(4, wv);
  uint64_t *res = s.dst<uint64_t>(4, wv);
  for (int x = lane; x < H; x += kWave) hits[x] = in[x];
  ANI_WAVE_SYNC();
  uint64_t k[KPT];
  l1_tiny_load_sort<uint64_t, KPT>(hits, H, k);     // (k_l1_tiny sorts 32-bit ranks through the same function)
#pragma unroll
  for (int r = 0; r < KPT; r++) hits[lane * KPT + r] = k[r];
  ANI_WAVE_SYNC();
  for (int x = lane; x < H; x += kWave) res[x] = hits[x];
}

__global__ __launch_bounds__(kTPB) void k_prim_rotl64(Slot s)
{
  const int n = s.n();
  const uint64_t *in = s.src<uint64_t>(1, 0);
  for (int i = threadIdx.x; i < n; i += kTPB) {
    const uint64_t x = in[i];
#pragma unroll
    for (int r = 1; r < 64; r++) s.dst<uint64_t>(63, r - 1)[i] = rotl64(x, r);     // unrolled: r is a constant, as at every call site
  }
}

__global__ __launch_bounds__(kTPB) void k_prim_perm(Slot s)
{
  const int n = s.n();
  const uint32_t *hi = s.src<uint32_t>(2, 0), *lo = s.src<uint32_t>(2, 1);
  uint32_t *res = s.dst<uint32_t>(1, 0);
  for (int j = threadIdx.x; j < n * kPermSelectors; j += kTPB) {
    const uint32_t i = (uint32_t)j / kPermSelectors, c = (uint32_t)j % kPermSelectors;
    const uint32_t sel = (c & 7u) | (((c >> 3) & 7u) << 8) | (((c >> 6) & 7u) << 16) | (((c >> 9) & 7u) << 24);
    res[j] = perm_b32(hi[i], lo[i], sel);
  }
}

__global__ __launch_bounds__(kTPB) void k_prim_alignbyte(Slot s)
{
  const int n = s.n();
  const uint32_t *hi = s.src<uint32_t>(3, 0), *lo = s.src<uint32_t>(3, 1), *by = s.src<uint32_t>(3, 2);
  uint32_t *res = s.dst<uint32_t>(1, 0);
  for (int i = threadIdx.x; i < n; i += kTPB) res[i] = alignbyte(hi[i], lo[i], by[i]);
}

// the largest sizes[b] the op's kernel stays inside its LDS array and its planes with
int max_size(int op, int cap)
{
  switch (op) {
    case OP_ARRAY_SCAN_LDS: case OP_ARRAY_SCAN_GLOBAL: return std::min(cap, kArrayScanCap);
    case OP_BLOCK_SORT_U32: case OP_BLOCK_SORT_U64: case OP_BITONIC_U32: case OP_BITONIC_U64: return std::min(cap, kBlockSortMax);
    case OP_WAVE_SORT_1: return std::min(cap, kWave);
    case OP_WAVE_SORT_2: return std::min(cap, 2 * kWave);
    case OP_WAVE_SORT_4: return std::min(cap, 4 * kWave);
    case OP_PERM_B32: return cap / kPermSelectors;
    default: return cap;                           // the per-thread ops ignore the size; cap >= threads is checked
  }
}
bool any_threads(int op) { return op == OP_WAVE_SCAN || op == OP_LANE_XOR_U32 || op == OP_LANE_XOR_U64 || op == OP_LANE_VALUE; }
}  // namespace

extern "C" int ani_prim_check(int op, const void *in, void *out, const int32_t *sizes, int blocks, int cap, int threads, hipStream_t stream)
{
  using anih::fail;
  if (op < 0 || op >= OP_N || !in || !out || !sizes || blocks < 0 || blocks > 65536) return fail(ANI_ERR_ARG, "ani_prim_check: bad argument");
  if (threads != kTPB && !(any_threads(op) && (threads == kWave || threads == 2 * kWave))) return fail(ANI_ERR_ARG, "ani_prim_check: op %d with %d threads",
      op, threads);
  if (cap < kTPB) return fail(ANI_ERR_ARG, "ani_prim_check: planes of %d elements", cap);
  if (blocks == 0) return ANI_OK;
  // the sizes are checked here, not in the kernels: a size beyond a kernel's array never reaches the device
  std::vector<int32_t> h((size_t)blocks);
  HIP_TRY(hipMemcpyAsync(h.data(), sizes, (size_t)blocks * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const int most = max_size(op, cap);
  for (int b = 0; b < blocks; b++)
    if (h[b] < 0 || h[b] > most) return fail(ANI_ERR_ARG, "ani_prim_check: op %d, size %d of workgroup %d is outside [0, %d]", op, h[b], b, most);
  const Slot s{in, out, sizes, cap};
  const dim3 g((unsigned)blocks), t((unsigned)threads);
  switch (op) {
    case OP_WAVE_SCAN: hipLaunchKernelGGL(k_prim_wave_scan, g, t, 0, stream, s); break;
    case OP_BLOCK_EXCL_SCAN: hipLaunchKernelGGL(k_prim_block_excl_scan, g, t, 0, stream, s); break;
    case OP_BLOCK_MAXSCAN: hipLaunchKernelGGL(k_prim_block_maxscan, g, t, 0, stream, s); break;
    case OP_ARRAY_SCAN_LDS: hipLaunchKernelGGL(k_prim_array_scan<false>, g, t, 0, stream, s); break;
    case OP_ARRAY_SCAN_GLOBAL: hipLaunchKernelGGL(k_prim_array_scan<true>, g, t, 0, stream, s); break;
    case OP_LANE_XOR_U32: hipLaunchKernelGGL(k_prim_lane_xor<uint32_t>, g, t, 0, stream, s); break;
    case OP_LANE_XOR_U64: hipLaunchKernelGGL(k_prim_lane_xor<uint64_t>, g, t, 0, stream, s); break;
    case OP_LANE_VALUE: hipLaunchKernelGGL(k_prim_lane_value, g, t, 0, stream, s); break;
    case OP_WAVE_UNIFORM_U32: hipLaunchKernelGGL(k_prim_wave_uniform<uint32_t>, g, t, 0, stream, s); break;
    case OP_WAVE_UNIFORM_U64: hipLaunchKernelGGL(k_prim_wave_uniform<uint64_t>, g, t, 0, stream, s); break;
    case OP_BLOCK_SORT_U32: hipLaunchKernelGGL((k_prim_block_sort<uint32_t, false>), g, t, 0, stream, s); break;
    case OP_BLOCK_SORT_U64: hipLaunchKernelGGL((k_prim_block_sort<uint64_t, false>), g, t, 0, stream, s); break;
    case OP_BITONIC_U32: hipLaunchKernelGGL((k_prim_block_sort<uint32_t, true>), g, t, 0, stream, s); break;
    case OP_BITONIC_U64: hipLaunchKernelGGL((k_prim_block_sort<uint64_t, true>), g, t, 0, stream, s); break;
    case OP_WAVE_SORT_1: hipLaunchKernelGGL(k_prim_wave_sort<1>, g, t, 0, stream, s); break;
    case OP_WAVE_SORT_2: hipLaunchKernelGGL(k_prim_wave_sort<2>, g, t, 0, stream, s); break;
    case OP_WAVE_SORT_4: hipLaunchKernelGGL(k_prim_wave_sort<4>, g, t, 0, stream, s); break;
    case OP_ROTL64: hipLaunchKernelGGL(k_prim_rotl64, g, t, 0, stream, s); break;
    case OP_PERM_B32: hipLaunchKernelGGL(k_prim_perm, g, t, 0, stream, s); break;
    default: hipLaunchKernelGGL(k_prim_alignbyte, g, t, 0, stream, s); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
  return ANI_OK;
}

extern "C" int ani_prim_device_scan(ani_ctx *ctx, const int32_t *in, uint32_t *out, uint32_t n, uint64_t *total, uint64_t limit)
{
  if (!ctx || !total) return anih::fail(ANI_ERR_ARG, "ani_prim_device_scan: null pointer");
  return anih::device_scan(ctx, in, out, n, total, limit);
}
