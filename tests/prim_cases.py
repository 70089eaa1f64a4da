"""Cases for the device primitives every kernel stands on (kernels/common.hpp: wave and workgroup scans, lane exchanges, the LDS and
register sorts, rotl64 / perm_b32 / alignbyte) and for the device-wide prefix sum (kernels/scan.hpp, device_scan in engine_core.hip),
run on their own through the test entry points of prim_check.hip and shared by the GPU tests (-m gpu, product library) and the
CPU-emulation tests (not gpu, tests/emu build): test_primitives.py.

Every case takes the loaded library (ctypes.CDLL) and `mem`, the triple (alloc, upload, download) of sort_cases.py.  The stream is
the null stream; device_scan runs on its context's stream and waits for it.

The references are numpy and Python integers written here: np.cumsum in int64 reduced mod 2^32, np.maximum.accumulate, np.sort,
index arithmetic for the lane functions, Python integers for rotl64 / perm_b32 / alignbyte.  No expected value comes from the library,
and every comparison is np.array_equal.

ani_prim_check runs one workgroup per slot (prim_check.hip has the table of ops).  A Launch collects one slot per (size,
distribution), so a primitive is checked in a handful of launches.  The input and output planes are handed over filled with
sort_cases.pattern; the whole output is compared with the pattern overlaid with the expected values, so anything written between the
slots, behind a slot's n-th element or behind the last slot fails the case, and the inputs must come back unchanged."""
import ctypes

import numpy as np

from sort_cases import GUARD, Buf, check_out, out_buf, pattern

WAVE, TPB = 64, 256
ERR_ARG, ERR_LIMIT = -1, -4                             # include/ani_abi.h
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

# name: (op code, element type, input planes, output planes) — the table of prim_check.hip
OPS = {name: (code, dtype, n_in, n_out) for code, (name, dtype, n_in, n_out) in enumerate((
    ("wave_scan", np.int32, 1, 2), ("block_excl_scan", np.int32, 2, 4), ("block_maxscan", np.int32, 2, 2), ("array_scan_lds", np.int32, 1, 2),
    ("array_scan_global", np.int32, 1, 2), ("lane_xor_u32", np.uint32, 1, 6), ("lane_xor_u64", np.uint64, 1, 6), ("lane_value", np.int32, 1, 5),
    ("wave_uniform_u32", np.uint32, 1, 2), ("wave_uniform_u64", np.uint64, 1, 2), ("block_sort_u32", np.uint32, 1, 1),
    ("block_sort_u64", np.uint64, 1, 1), ("bitonic_u32", np.uint32, 1, 1), ("bitonic_u64", np.uint64, 1, 1), ("wave_sort_1", np.uint64, 4, 4),
    ("wave_sort_2", np.uint64, 4, 4), ("wave_sort_4", np.uint64, 4, 4), ("rotl64", np.uint64, 1, 63), ("perm_b32", np.uint32, 2, 1),
    ("alignbyte", np.uint32, 3, 1)))}
ANY_THREADS = (WAVE, 2 * WAVE, TPB)                     # the wave-level ops run with one, two and four waves

# every switch arm of block_sort (64 .. 4096 keys), one-wave and four-wave, on both sides of each
SORT_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
BITONIC_SIZES = tuple(sorted(set(SORT_SIZES) | {1 << k for k in range(1, 13)}))     # block_bitonic_sort: n2 = 2 .. 4096
SORT_DISTS = ("uniform", "equal", "two", "sorted", "reverse", "padding", "high", "low")
WAVE_SORT_SIZES = {1: (0, 1, 2, 33, 63, 64), 2: (1, 64, 65, 100, 127, 128), 4: (1, 64, 128, 129, 200, 255, 256)}    # l1_tiny_sort<KPT>: H <= 64 KPT
# the 8-per-thread and the 2048-per-pass borders of block_array_excl_scan
ARRAY_SCAN_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4097, 6000)
SCAN_DISTS = ("zeros", "ones", "lane63", "wave1", "last", "first", "negative", "wrap", "uniform")
MAX_DISTS = SCAN_DISTS + ("sentinel", "full", "descending")
SCAN_BLOCK = 2048                                       # kernels/scan.hpp: kScanPerBlock
# device_scan: the block borders, and more blocks than the device runs at once
DEVICE_SCAN_SIZES = (1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 3 * SCAN_BLOCK + 5, 300 * SCAN_BLOCK + 1)
DEVICE_SCAN_DISTS = ("uniform", "zeros", "ones", "borders")
DEFAULT_LIMIT = 0xfffffff0                              # host/engine.hpp: device_scan's default limit, 2^32 - 16


def bind(lib):
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.ani_prim_check.argtypes = [i, vp, vp, vp, i, i, i, vp]
    lib.ani_prim_device_scan.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64]
    lib.ani_prim_check.restype = lib.ani_prim_device_scan.restype = i
    return lib


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def wrap32(a):
    """int64 sums reduced mod 2^32, as the int32 the device holds"""
    return (np.asarray(a, dtype=np.int64) & M32).astype(np.uint32).view(np.int32)


# ---- one launch of ani_prim_check ----
class Launch:
    """the slots of one call: add(label, inputs, expected, n) per workgroup, then run()"""

    def __init__(self, op, threads=TPB):
        self.op, self.threads = op, threads
        self.code, self.dtype, self.n_in, self.n_out = OPS[op]
        self.slots = []

    def add(self, label, inputs, expected, n=0):
        """inputs: one array per input plane; expected: one array per output plane, the elements the workgroup must write (from the
        plane's first on); n: the slot's entry of `sizes`"""
        assert len(inputs) == self.n_in and len(expected) == self.n_out, self.op
        self.slots.append((label, [np.asarray(a, dtype=self.dtype) for a in inputs], [np.asarray(a, dtype=self.dtype) for a in expected], n))

    def run(self, lib, mem, runs=1):
        """`runs` > 1 repeats the call into fresh outputs, which must all be right (and therefore equal)"""
        nb = len(self.slots)
        cap = max([TPB] + [len(a) for _, ins, exp, _ in self.slots for a in ins + exp]) + GUARD
        host_in = pattern(nb * self.n_in * cap, self.dtype, 3).reshape(nb, self.n_in, cap)
        for b, (_, ins, _, _) in enumerate(self.slots):
            for p, a in enumerate(ins):
                host_in[b, p, :len(a)] = a
        d_in = Buf(mem, host_in)
        d_sizes = Buf(mem, np.array([n for _, _, _, n in self.slots], dtype=np.int32))
        for run in range(runs):
            d_out = Buf(mem, pattern(nb * self.n_out * cap + GUARD, self.dtype, 5 + run))
            rc = lib.ani_prim_check(self.code, d_in.ptr, d_out.ptr, d_sizes.ptr, nb, cap, self.threads, None)
            assert rc == 0, "%s: ani_prim_check returned %d" % (self.op, rc)
            want = d_out.init.copy()
            planes = want[:nb * self.n_out * cap].reshape(nb, self.n_out, cap)
            for b, (_, _, exp, _) in enumerate(self.slots):
                for p, a in enumerate(exp):
                    planes[b, p, :len(a)] = a
            got = d_out.get()
            if not np.array_equal(got, want):
                self._report(got, want, cap, run)
            assert d_in.unchanged() and d_sizes.unchanged(), "%s: an input was written" % self.op

    def _report(self, got, want, cap, run):
        bad = np.flatnonzero(got != want)
        at = int(bad[0])
        if at >= len(self.slots) * self.n_out * cap:
            raise AssertionError("%s: written behind the last slot" % self.op)
        b, p, i = at // (self.n_out * cap), at // cap % self.n_out, at % cap
        label, _, exp, n = self.slots[b]
        where = "element %d is wrong" % i if i < len(exp[p]) else "written behind its %d elements, at %d" % (len(exp[p]), i)
        raise AssertionError("%s, %d threads, run %d: %d elements differ, the first in slot %d (%s, n = %d), output %d: %s (got %r, want %r)" % (
            self.op, self.threads, run, len(bad), b, label, n, p, where, got[at], want[at]))


# ---- scans ----
def scan_values(dist, n, seed=0):
    """n int32 values.  The single non-zero value sits where a scan hands over: the last lane of wave 0, the first lane of wave 1,
    the last and the first thread (for the array scan: the same places in units of elements)"""
    r = rng(seed, n, MAX_DISTS.index(dist))
    v = np.zeros(n, dtype=np.int64)
    if dist == "ones":
        v[:] = 1
    elif dist in ("lane63", "wave1", "last", "first"):
        at = {"lane63": WAVE - 1, "wave1": WAVE, "last": n - 1, "first": 0}[dist]
        if 0 <= at < n:
            v[at] = 0x12345
    elif dist == "negative":                            # the sums go below zero and come back
        v = r.integers(-1000, 1001, n)
    elif dist == "wrap":                                # a wave's sum passes 2^31 several times
        v = r.integers(1 << 27, 1 << 28, n)
    elif dist == "uniform":
        v = r.integers(0, 1000, n)
    elif dist == "sentinel":                            # the max scan's callers: -1 = "no predecessor", a few real positions
        v[:] = -1
        if n:
            at = r.integers(0, n, max(1, n // 40))
            v[at] = r.integers(0, 1 << 20, len(at))
    elif dist == "full":
        v = r.integers(-(1 << 31), 1 << 31, n)
    elif dist == "descending":
        v = -np.sort(-r.integers(-(1 << 31), 1 << 31, n))
    return v.astype(np.int32)


def excl_scan(v):
    """(exclusive prefix sums, total), both mod 2^32"""
    c = np.cumsum(v, dtype=np.int64)
    return wrap32(c - v), wrap32(c[-1:] if len(v) else np.zeros(1))[0]


def case_wave_scans(lib, mem, threads, dists=SCAN_DISTS):
    """wave_incl_scan and wave_incl_scan_dpp, every wave of the workgroup with its own data"""
    launch = Launch("wave_scan", threads)
    for dist in dists:
        v = scan_values(dist, threads, seed=1)
        if dist in ("lane63", "first"):                 # ... in every wave
            v = np.tile(v[:WAVE], threads // WAVE)
        incl = wrap32(np.cumsum(v.reshape(-1, WAVE), axis=1, dtype=np.int64)).reshape(-1)
        launch.add(dist, [v], [incl, incl])
    launch.run(lib, mem)


def case_block_excl_scan(lib, mem, dists=SCAN_DISTS):
    """two calls in a row on one scratch array: the second call's data is the next distribution's"""
    launch = Launch("block_excl_scan")
    for k, dist in enumerate(dists):
        v0, v1 = scan_values(dist, TPB, seed=2), scan_values(dists[(k + 1) % len(dists)], TPB, seed=3)
        (e0, t0), (e1, t1) = excl_scan(v0), excl_scan(v1)
        launch.add(dist, [v0, v1], [e0, np.full(TPB, t0), e1, np.full(TPB, t1)])    # every thread gets the total
    launch.run(lib, mem)


def case_block_maxscan(lib, mem, dists=MAX_DISTS):
    launch = Launch("block_maxscan")
    for k, dist in enumerate(dists):
        v0, v1 = scan_values(dist, TPB, seed=4), scan_values(dists[(k + 1) % len(dists)], TPB, seed=5)
        launch.add(dist, [v0, v1], [np.maximum.accumulate(v0), np.maximum.accumulate(v1)])
    launch.run(lib, mem)


def case_array_scan(lib, mem, where, sizes=ARRAY_SCAN_SIZES, dists=SCAN_DISTS):
    """block_array_excl_scan over an array in LDS ("lds") or in global memory ("global")"""
    launch = Launch("array_scan_" + where)
    for n in sizes:
        for dist in dists:
            v = scan_values(dist, n, seed=6)
            if dist in ("lane63", "wave1") and n > 8 * WAVE:     # the elements of thread 63 / thread 64, and the pass border
                v = np.zeros(n, dtype=np.int32)
                v[8 * WAVE - 1 if dist == "lane63" else 8 * WAVE] = 0x12345
                v[min(n - 1, SCAN_BLOCK - 1 if dist == "lane63" else SCAN_BLOCK)] = 0x6789
            e, t = excl_scan(v)
            launch.add("%s n=%d" % (dist, n), [v], [e, np.full(TPB, t)], n)
    launch.run(lib, mem)


# ---- lane exchanges ----
def lane_data(dtype, threads, kind, seed):
    r = rng(seed, threads)
    if dtype == np.uint32 or dtype == np.int32:
        return r.integers(0, 1 << 32, threads, dtype=np.uint64).astype(np.uint32).view(dtype)
    hi, lo = r.integers(0, 1 << 32, threads, dtype=np.uint64), r.integers(0, 1 << 32, threads, dtype=np.uint64)
    if kind == "high":                                  # the halves travel separately: lanes that differ in one half only
        lo[:] = 0x89abcdef
    if kind == "low":
        hi[:] = 0x01234567
    return (hi << np.uint64(32)) | lo


def case_lane_xor(lib, mem, bits, threads):
    """lane_xor<M>, M = 1 .. 32: the value of lane ^ M, in every wave"""
    dtype = np.uint32 if bits == 32 else np.uint64
    launch = Launch("lane_xor_u%d" % bits, threads)
    t = np.arange(threads)
    for kind in ("uniform",) if bits == 32 else ("uniform", "high", "low"):
        x = lane_data(dtype, threads, kind, seed=7)
        launch.add(kind, [x], [x[t ^ (1 << m)] for m in range(6)])
    launch.add("lane number", [t], [t ^ (1 << m) for m in range(6)])
    launch.run(lib, mem)


def case_lane_value(lib, mem, threads):
    """lane_value(x, l): what lane l of the thread's own wave holds, l = 0, 1, 31, 32, 63"""
    launch = Launch("lane_value", threads)
    for seed in (8, 9):
        x = lane_data(np.int32, threads, "uniform", seed)
        launch.add("uniform", [x], [np.repeat(x.reshape(-1, WAVE)[:, l], WAVE) for l in (0, 1, 31, 32, 63)])
    launch.run(lib, mem)


def case_wave_uniform(lib, mem, bits):
    """wave_uniform(x) of a value that is the same in every lane of the wave gives x, with all lanes and with some"""
    dtype = np.uint32 if bits == 32 else np.uint64
    launch = Launch("wave_uniform_u%d" % bits)
    lane = np.arange(TPB) % WAVE
    for kind in ("uniform",) if bits == 32 else ("uniform", "high", "low"):
        x = lane_data(dtype, TPB // WAVE, kind, seed=10)
        every = np.repeat(x, WAVE)
        launch.add(kind, [x], [every, np.where(lane % 4 == 1, every, ~every)])
    launch.run(lib, mem)


# ---- sorts ----
def sort_keys(dist, n, dtype, seed=0):
    """n keys; "high" and "low" (64-bit keys only) differ in one 32-bit half only"""
    bits = 8 * np.dtype(dtype).itemsize
    r = rng(seed, n, bits, SORT_DISTS.index(dist))
    keys = r.integers(0, 1 << bits, n, dtype=np.uint64)
    if dist == "equal":
        keys[:] = r.integers(0, 1 << bits, dtype=np.uint64)
    elif dist == "two":
        keys = r.integers(0, 1 << bits, 2, dtype=np.uint64)[r.integers(0, 2, n)]
    elif dist == "sorted":
        keys = np.sort(keys)
    elif dist == "reverse":
        keys = np.sort(keys)[::-1].copy()
    elif dist == "padding" and n:                       # keys equal to the padding value ~0, and its neighbour ~0 - 1
        keys[r.integers(0, n, max(1, n // 4))] = (1 << bits) - 1
        keys[r.integers(0, n, max(1, n // 8))] = (1 << bits) - 2
        keys[r.integers(0, n)] = (1 << bits) - 1
    elif dist == "high":
        keys = (keys & np.uint64(0xffffffff00000000)) | np.uint64(0x89abcdef)
    elif dist == "low":
        keys = (keys & np.uint64(M32)) | np.uint64(0x0123456700000000)
    return keys.astype(dtype)


def dists_of(bits, dists):
    return [d for d in dists if bits == 64 or d not in ("high", "low")]


def case_block_sort(lib, mem, network, bits, sizes=None, dists=SORT_DISTS, runs=1):
    """block_sort ("block_sort": the register network behind its switch) or block_bitonic_sort ("bitonic": the LDS network)"""
    dtype = np.uint32 if bits == 32 else np.uint64
    launch = Launch("%s_u%d" % (network, bits))
    for n in sizes if sizes is not None else (SORT_SIZES if network == "block_sort" else BITONIC_SIZES):
        for dist in dists_of(bits, dists):
            keys = sort_keys(dist, n, dtype, seed=11)
            launch.add("%s n=%d" % (dist, n), [keys], [np.sort(keys)], n)
    launch.run(lib, mem, runs)


def case_wave_sort(lib, mem, kpt, sizes=None, dists=SORT_DISTS):
    """wave_sort_regs<uint64_t, KPT> as l1_tiny_sort<KPT> runs it: each of the four waves sorts its own H keys at the same time"""
    launch = Launch("wave_sort_%d" % kpt)
    for n in sizes if sizes is not None else WAVE_SORT_SIZES[kpt]:
        for dist in dists:
            keys = [sort_keys(dist, n, np.uint64, seed=20 + w) for w in range(TPB // WAVE)]
            launch.add("%s H=%d" % (dist, n), keys, [np.sort(k) for k in keys], n)
    launch.run(lib, mem)


# ---- element-wise helpers ----
WORDS64 = [0, 1, 1 << 63, M64, 0x0123456789abcdef, 0x00000000ffffffff, 0xffffffff00000000, 0x8000000000000001, 0x00000001fffffffe]
WORD_PAIRS = [(0x07060504, 0x03020100), (0xfedcba98, 0x76543210), (0x80ff7f01, 0x00fe8102), (0xffffffff, 0x00000000)]


def case_rotl64(lib, mem):
    """rotl64(x, r), r = 1 .. 63"""
    words = WORDS64 + [int(x) for x in rng(12).integers(0, 1 << 64, 60, dtype=np.uint64)]
    launch = Launch("rotl64")
    launch.add("words", [np.array(words, dtype=np.uint64)],
               [np.array([((x << r) | (x >> (64 - r))) & M64 for x in words], dtype=np.uint64) for r in range(1, 64)], len(words))
    launch.run(lib, mem)


def case_perm_b32(lib, mem):
    """perm_b32(hi, lo, sel): result byte j = byte sel_j of the eight bytes {hi, lo}, all 4096 selectors of bytes 0 .. 7"""
    pairs = WORD_PAIRS + [(int(a), int(b)) for a, b in rng(13).integers(0, 1 << 32, (2, 2), dtype=np.uint64)]
    want = []
    for hi, lo in pairs:
        src = (hi << 32) | lo
        for c in range(4096):
            want.append(sum(((src >> (8 * ((c >> (3 * j)) & 7))) & 0xff) << (8 * j) for j in range(4)))
    launch = Launch("perm_b32")
    launch.add("pairs", [np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)],
               [np.array(want, dtype=np.uint32)], len(pairs))
    launch.run(lib, mem)


def case_alignbyte(lib, mem):
    """alignbyte(hi, lo, n): the 32 bits of {hi, lo} that start n bytes up, n = 0 .. 3"""
    pairs = WORD_PAIRS + [(int(a), int(b)) for a, b in rng(14).integers(0, 1 << 32, (60, 2), dtype=np.uint64)]
    args = [(hi, lo, n) for hi, lo in pairs for n in range(4)]
    launch = Launch("alignbyte")
    launch.add("pairs", [np.array([a[k] for a in args], dtype=np.uint32) for k in range(3)],
               [np.array([((((hi << 32) | lo) >> (8 * n)) & M32) for hi, lo, n in args], dtype=np.uint32)], len(args))
    launch.run(lib, mem)


def case_arguments(lib, mem):
    """sizes beyond a check kernel's arrays, thread counts it is not written for and unknown ops are refused before anything runs"""
    for op, threads, n in (("block_sort_u64", TPB, 4097), ("bitonic_u32", TPB, 4097), ("array_scan_lds", TPB, 6145), ("wave_sort_1", TPB, 65),
                           ("wave_sort_4", TPB, 257), ("perm_b32", TPB, 2), ("block_sort_u32", TPB, -1), ("block_excl_scan", WAVE, 0),
                           ("block_sort_u64", 2 * WAVE, 0), ("lane_xor_u32", 32, 0), ("lane_xor_u32", 512, 0), (None, TPB, 0)):
        code, dtype, n_in, n_out = OPS[op] if op else (len(OPS), np.uint32, 1, 1)
        cap = 4096 + GUARD
        d_in, d_out = Buf(mem, pattern(n_in * cap, dtype, 41)), Buf(mem, pattern(n_out * cap, dtype, 42))
        d_sizes = Buf(mem, np.array([n], dtype=np.int32))
        rc = lib.ani_prim_check(code, d_in.ptr, d_out.ptr, d_sizes.ptr, 1, cap, threads, None)
        assert rc == ERR_ARG, "%s with %d threads, n = %d: returned %d" % (op, threads, n, rc)
        assert d_out.unchanged() and d_in.unchanged(), "%s: a refused call wrote something" % op


# ---- device_scan ----
def counts_with_total(n, total, seed=0):
    """n counts >= 0 around total / n (+- 10 %) that add up to `total` exactly"""
    mean = total // n
    c = mean + rng(seed, n, total).integers(-(mean // 10), mean // 10 + 1, n)
    d = total - int(c.sum())
    c += d // n                                         # (spread over all counts: the last one alone could go below zero)
    c[-1] += d - d // n * n
    assert int(c.sum()) == total and c.min() >= 0 and c.max() < 1 << 31
    for b in range(0, n, SCAN_BLOCK):                   # k_scan_blocks adds a block up in int32
        assert int(c[b:b + SCAN_BLOCK].sum()) < 1 << 31
    return c.astype(np.int32)


def scan_counts(dist, n, seed=0):
    r = rng(seed, n, DEVICE_SCAN_DISTS.index(dist))
    if dist == "uniform":
        return r.integers(0, 1000, n).astype(np.int32)
    c = np.full(n, 1 if dist == "ones" else 0, dtype=np.int32)
    if dist == "borders":                               # the last element of block 0, the first of block 1, the last of all
        for at, v in ((SCAN_BLOCK - 1, 0x12345), (SCAN_BLOCK, 0x6789), (n - 1, 0x1111)):
            if at < n:
                c[at] += v
    return c


def device_scan(lib, mem, ctx, counts, limit=DEFAULT_LIMIT, runs=1):
    """One ani_prim_device_scan of `counts`: offsets and *total exact when the total is within `limit`, ANI_ERR_LIMIT and *total == 0
    beyond it.  Nothing is written behind the n-th offset either way; the counts come back unchanged."""
    n = len(counts)
    total = int(counts.astype(np.int64).sum())
    what = "device_scan n=%d total=%d limit=%d" % (n, total, limit)
    d_in = Buf(mem, counts)
    for run in range(runs):
        d_out = out_buf(mem, n, np.uint32, 61 + run)
        got = ctypes.c_uint64(0xdeadbeefdeadbeef)
        rc = lib.ani_prim_device_scan(ctx, d_in.ptr, d_out.ptr, n, ctypes.byref(got), limit)
        if total > limit:
            assert rc == ERR_LIMIT, "%s: returned %d, not ANI_ERR_LIMIT" % (what, rc)
            assert got.value == 0, "%s: *total = %d after ANI_ERR_LIMIT" % (what, got.value)
            assert np.array_equal(d_out.get()[n:], d_out.init[n:]), "%s: written behind the %d-th element" % (what, n)
        else:
            assert rc == 0, "%s: returned %d" % (what, rc)
            assert got.value == total, "%s: *total = %d" % (what, got.value)
            c = np.cumsum(counts, dtype=np.int64)
            check_out(d_out, n, ((c - counts) & M32).astype(np.uint32), what)
        assert d_in.unchanged(), "%s: the counts were written" % what


def case_device_scan(lib, mem, ctx, n, dists=DEVICE_SCAN_DISTS):
    for dist in dists:
        device_scan(lib, mem, ctx, scan_counts(dist, n, seed=30))


def case_device_scan_empty(lib, mem, ctx):
    """n = 0: total 0, nothing touched (the pointers are not even looked at)"""
    device_scan(lib, mem, ctx, np.zeros(0, dtype=np.int32))
    got = ctypes.c_uint64(7)
    assert lib.ani_prim_device_scan(ctx, None, None, 0, ctypes.byref(got), DEFAULT_LIMIT) == 0 and got.value == 0


def case_device_scan_large_totals(lib, mem, ctx, n):
    """block totals below 2^31, the grand total between 2^31 and 2^32 - 16: offsets beyond 2^31 must be exact"""
    for total in ((1 << 31) + 12345, 3000000001, DEFAULT_LIMIT - 1, DEFAULT_LIMIT):
        device_scan(lib, mem, ctx, counts_with_total(n, total, seed=31))


def case_device_scan_default_limit(lib, mem, ctx, n=3 * SCAN_BLOCK + 5):
    """a total just above 2^32 - 16, and one that 32 bits would have wrapped to a small number, give ANI_ERR_LIMIT and *total == 0; the
    context gives right answers after every refusal (the pinned staging buffer and the block-total buffers are shared state)"""
    ok = scan_counts("uniform", n, seed=32)
    for total in (DEFAULT_LIMIT + 1, (1 << 32) + 5):
        device_scan(lib, mem, ctx, counts_with_total(n, total, seed=33))
        device_scan(lib, mem, ctx, ok)


def case_device_scan_caller_limit(lib, mem, ctx, n):
    """the limit is inclusive: with a caller's limit L a total of L passes and L + 1 fails, and the context works on after it"""
    limits = (5 * n, 1000003) + (((1 << 31) + 7,) if n > 2 * SCAN_BLOCK else ())
    for limit in limits:
        device_scan(lib, mem, ctx, counts_with_total(n, limit, seed=34), limit)
        device_scan(lib, mem, ctx, counts_with_total(n, limit + 1, seed=34), limit)
        device_scan(lib, mem, ctx, counts_with_total(n, limit, seed=35), limit)
        device_scan(lib, mem, ctx, counts_with_total(n, limit - 1, seed=34), limit)
    device_scan(lib, mem, ctx, np.zeros(n, dtype=np.int32), 0)                      # limit 0: only a total of 0 passes
    device_scan(lib, mem, ctx, scan_counts("borders", n, seed=36), 0)
    device_scan(lib, mem, ctx, scan_counts("uniform", n, seed=32))


def case_determinism_sort(lib, mem, n=SORT_SIZES[-1]):
    """the largest sort case three times into fresh outputs: all right, hence equal"""
    case_block_sort(lib, mem, "block_sort", 64, sizes=(n,), dists=("uniform", "two"), runs=3)
    case_block_sort(lib, mem, "bitonic", 64, sizes=(n,), dists=("uniform", "two"), runs=3)


def case_determinism_scan(lib, mem, ctx, n=DEVICE_SCAN_SIZES[-1]):
    device_scan(lib, mem, ctx, counts_with_total(n, 3000000001, seed=37), runs=3)
