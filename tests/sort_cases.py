"""Cases for the device radix sort (kernels/radix.hpp, sort_device.hip), called directly through its extern "C" entry points and
shared by the GPU tests (-m gpu, product library) and the CPU-emulation tests (not gpu, tests/emu build): test_radix_sort.py.

Every case takes the loaded library (ctypes.CDLL) and `mem`, a triple (alloc, upload, download):
    alloc(nbytes)      -> (buffer, address)          device memory of nbytes bytes
    upload(buffer, a)                                 a: numpy uint8 array of the buffer's size; complete when it returns
    download(buffer)   -> numpy uint8 array           waits for the device first
The stream is the null stream.

The reference is numpy on the host: np.argsort(bits [beginBit, endBit) of the key, kind="stable"); the whole key and the payload
follow that permutation.  Every comparison is np.array_equal: a stable sort has exactly one right answer.

Every call follows the two-phase contract of the entry points (tmp = NULL: the workspace size, nothing touched; then a workspace
of that size + 256 bytes, as the callers in engine_*.hip allocate it), and every case checks what the sort writes besides its
result: the elements behind an output's n-th, the inputs, and the bytes in front of and behind the workspace must keep their
patterns.  The workspace itself is handed over filled with a pattern: the sort zeroes what it needs zeroed."""
import ctypes

import numpy as np

WAVE, WORKGROUP, TILE = 64, 512, 6144                   # kernels/radix.hpp: 512 threads x 12 keys per tile
SIZES = (1, 2, WAVE - 1, WAVE, WAVE + 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1,
         3 * TILE + 777)
# several times the workgroups the device holds at once: later tiles start while earlier ones have not published their prefixes
BIG_SIZE = 1500 * TILE + 1
# (beginBit, endBit): 8, 1, 1, 1, 2, 1, 3, 2, 5, 5 and 1 passes — odd and even counts take the two directions of the ping-pong
RANGES = ((0, 64), (0, 1), (63, 64), (0, 8), (0, 9), (5, 6), (7, 24), (31, 47), (31, 64), (0, 40), (56, 64))
END_BITS = tuple(e for b, e in RANGES if b == 0)        # ani_sort_keys_u64_bits / ani_sort_pairs_u64_u32 sort the bits [0, endBit)
DISTS = ("uniform", "three", "equal", "rare", "sorted", "reverse")
INDEX_DISTS = ("min24", "repeats")

GUARD = 64                                              # elements behind every array's n-th
FENCE = 1024                                            # bytes in front of and behind the workspace
ERR_SIZE, ERR_WORKSPACE, ERR_PIECES, ERR_BEGIN_BIT = 9002, 9003, 9004, 9005


def bind(lib):
    """argtypes of the sort's entry points (size_t and pointers must not travel as default ints)"""
    vp, sz, i, psz = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)
    lib.ani_sort_keys_u64_range.argtypes = [vp, vp, sz, i, i, vp, psz, vp, i]
    lib.ani_sort_keys_u64_bits.argtypes = [vp, vp, sz, i, vp, psz, vp]
    lib.ani_sort_pairs_u64_u32.argtypes = [vp, vp, vp, vp, sz, i, vp, psz, vp]
    lib.ani_sort_index.argtypes = [ctypes.POINTER(vp), psz, i, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp, vp, psz, vp, vp, vp]
    lib.ani_sort_check.argtypes = [vp, vp]
    for f in (lib.ani_sort_keys_u64_range, lib.ani_sort_keys_u64_bits, lib.ani_sort_pairs_u64_u32, lib.ani_sort_index, lib.ani_sort_check):
        f.restype = i
    return lib


# ---- reference ----
def masked(keys, begin, end):
    """bits [begin, end) of the keys, in the narrowest unsigned type that holds them"""
    width = end - begin
    m = keys >> np.uint64(begin)
    if width < 64:
        m = m & np.uint64((1 << width) - 1)
    for bits, t in ((8, np.uint8), (16, np.uint16), (32, np.uint32)):
        if width <= bits:
            return m.astype(t)
    return m


def stable_order(keys, begin, end):
    return np.argsort(masked(keys, begin, end), kind="stable")


# ---- inputs ----
def pattern(n, dtype, salt):
    """a known filling for memory that must not be written (or must be written completely): no two neighbours alike"""
    return ((np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(7)).astype(dtype)


def make_keys(dist, n, begin, end, seed=0):
    """n 64-bit keys whose bits [begin, end) follow `dist`; every other bit is random, so a sort that looks at them, drops them or
    is not stable gives a different array"""
    r = np.random.default_rng([seed, n, begin, end, DISTS.index(dist)])
    width = end - begin
    field = np.uint64((1 << width) - 1) << np.uint64(begin)
    keys = r.integers(0, 1 << 64, n, dtype=np.uint64)

    def with_field(values):
        return (keys & ~field) | ((values.astype(np.uint64) << np.uint64(begin)) & field)

    if dist == "uniform":
        return keys
    if dist == "three":                                 # three values of the sorted bits (two when there is one bit), ~n / 3 times each
        choice = r.integers(0, 1 << 64, min(3, 1 << width), dtype=np.uint64) >> np.uint64(64 - width)
        if len(set(choice.tolist())) < len(choice):
            choice = np.arange(len(choice), dtype=np.uint64)
        return with_field(choice[r.integers(0, len(choice), n)])
    if dist == "equal":                                 # one digit's run spans every tile, in every pass
        return with_field(np.full(n, r.integers(0, 1 << 64, dtype=np.uint64) >> np.uint64(64 - width)))
    if dist == "rare":                                  # the sorted bits all ones in one key of the first tile and one of the last, 0 elsewhere:
        v = np.zeros(n, dtype=np.uint64)                # the last tile's look-back for that digit walks the whole chain of zero aggregates
        v[min(n - 1, 100)] = v[n - 1 - min(n - 1, 37)] = (1 << width) - 1
        return with_field(v)
    order = stable_order(keys, begin, end)              # ties stay in a random order of the other bits
    return keys[order] if dist == "sorted" else keys[order[::-1]]


def make_records(dist, n, seq_base, seed=0):
    """n minimizer records (hash, seqId, wpos) in position order, seqIds from seq_base on"""
    r = np.random.default_rng([seed, n, INDEX_DISTS.index(dist)])
    if dist == "min24":                                 # a window minimizer is the smallest of ~24 hashes: the top digit takes few values
        h = np.full(n, 0xffffffff, dtype=np.uint32)
        for _ in range(24):
            np.minimum(h, r.integers(0, 1 << 32, n, dtype=np.uint32), out=h)
    else:                                               # few hashes, hundreds of occurrences each, all over the pieces
        pool = r.integers(0, 1 << 32, max(1, n // 300), dtype=np.uint32)
        h = pool[r.integers(0, len(pool), n)]
    i = np.arange(n, dtype=np.uint64)
    per_seq = max(1, n // 5 + 1)                        # five contigs
    rec = np.empty((n, 3), dtype=np.uint32)
    rec[:, 0] = h
    rec[:, 1] = seq_base + i // per_seq
    rec[:, 2] = 3 + 7 * (i % per_seq)
    return rec


def split_pieces(n):
    """piece sizes that add up to n: no piece ends on a tile border (unless n itself does), one piece is empty"""
    cuts = []
    for c in (n // 3, n // 3 + TILE + 5, (7 * n) // 8):
        c += 1 if c % TILE == 0 else 0
        if 0 < c < n and c not in cuts:
            cuts.append(c)
    edges = [0] + sorted(cuts) + [n]
    sizes = [edges[k + 1] - edges[k] for k in range(len(edges) - 1)]
    sizes.insert(1, 0)
    return sizes


# ---- device memory with patterns around it ----
class Buf:
    """a device buffer that starts as `init`"""

    def __init__(self, mem, init):
        self.mem, self.init = mem, init
        self.buf, self.ptr = mem[0](max(init.nbytes, 8))
        if init.nbytes:
            host = np.zeros(max(init.nbytes, 8), dtype=np.uint8)
            host[:init.nbytes] = init.reshape(-1).view(np.uint8)
            mem[1](self.buf, host)

    def get(self):
        return self.mem[2](self.buf)[:self.init.nbytes].view(self.init.dtype).reshape(self.init.shape)

    def unchanged(self):
        return np.array_equal(self.get(), self.init)


def out_buf(mem, n, dtype, salt):
    return Buf(mem, pattern(n + GUARD, dtype, salt))


def check_out(buf, n, expected, what):
    """the first n elements are the result, the rest still the pattern"""
    got = buf.get()
    assert np.array_equal(got[n:], buf.init[n:]), "%s: written behind the %d-th element" % (what, n)
    if not np.array_equal(got[:n], expected):
        bad = np.flatnonzero(got[:n] != expected)
        raise AssertionError("%s: %d of %d elements differ, the first at %d, the last at %d" % (what, len(bad), n, bad[0], bad[-1]))


class Workspace:
    """`nbytes` + 256 bytes of workspace between two fences, all of it patterned"""

    def __init__(self, mem, nbytes):
        self.room = nbytes + 256
        self.all = Buf(mem, pattern(FENCE + self.room + FENCE, np.uint8, 0x55))
        self.ptr = self.all.ptr + FENCE

    def check_fences(self, what):
        got = self.all.get()
        assert np.array_equal(got[:FENCE], self.all.init[:FENCE]), "%s: written in front of the workspace" % what
        assert np.array_equal(got[FENCE + self.room:], self.all.init[FENCE + self.room:]), "%s: written behind the workspace" % what


# ---- the array sorts ----
def array_sort(lib, mem, entry, keys, begin, end, runs=1, use_async=False, norm=None):
    """One sort of `keys` by ani_sort_keys_u64_range ("range"), ani_sort_keys_u64_bits ("bits") or ani_sort_pairs_u64_u32 ("pairs";
    payload arange(n), so that the payload that comes back is the permutation), checked against the reference.  `runs` > 1 repeats
    the sort into fresh outputs, which must be byte-equal.  `norm`: the range the arguments are expected to be read as."""
    n = len(keys)
    what = "%s n=%d bits [%d, %d)" % (entry, n, begin, end)
    pairs = entry == "pairs"
    assert entry == "range" or begin == 0
    k_in = Buf(mem, keys)
    v_in = Buf(mem, np.arange(n, dtype=np.uint32)) if pairs else None

    def call(k_out, v_out, tmp, tmp_bytes):
        if entry == "range":
            return lib.ani_sort_keys_u64_range(k_in.ptr, k_out.ptr, n, begin, end, tmp, ctypes.byref(tmp_bytes), None, 1 if use_async else 0)
        if entry == "bits":
            return lib.ani_sort_keys_u64_bits(k_in.ptr, k_out.ptr, n, end, tmp, ctypes.byref(tmp_bytes), None)
        return lib.ani_sort_pairs_u64_u32(k_in.ptr, k_out.ptr, v_in.ptr, v_out.ptr, n, end, tmp, ctypes.byref(tmp_bytes), None)

    order = stable_order(keys, *(norm or (begin, end)))
    first = None
    for run in range(runs):
        k_out = out_buf(mem, n, np.uint64, 1 + run)
        v_out = out_buf(mem, n, np.uint32, 11 + run) if pairs else None
        tmp_bytes = ctypes.c_size_t(0)
        assert call(k_out, v_out, None, tmp_bytes) == 0, what
        assert tmp_bytes.value > 0, what
        assert k_out.unchanged() and (not pairs or v_out.unchanged()), "%s: the size query wrote to an output" % what
        ws = Workspace(mem, tmp_bytes.value)
        rc = call(k_out, v_out, ws.ptr, tmp_bytes)
        assert rc == 0, "%s: returned %d" % (what, rc)
        if use_async:
            rc = lib.ani_sort_check(ws.ptr, None)
            assert rc == 0, "%s: ani_sort_check returned %d" % (what, rc)
        check_out(k_out, n, keys[order], what + " keys")
        if pairs:
            check_out(v_out, n, order.astype(np.uint32), what + " payload")
        ws.check_fences(what)
        assert k_in.unchanged() and (not pairs or v_in.unchanged()), "%s: an input was written" % what
        got = (k_out.get()[:n].tobytes(), v_out.get()[:n].tobytes() if pairs else b"")
        if first is None:
            first = got
        assert got == first, "%s: run %d differs from run 0" % (what, run)


def case_array(lib, mem, entry, n, bit_range, dist):
    begin, end = bit_range
    array_sort(lib, mem, entry, make_keys(dist, n, begin, end), begin, end)


def case_async(lib, mem, n=2 * TILE + 1):
    """ani_sort_keys_u64_range with async = 1 returns with the passes in flight; ani_sort_check completes it"""
    for begin, end in ((31, 47), (31, 64)):
        array_sort(lib, mem, "range", make_keys("three", n, begin, end, seed=3), begin, end, use_async=True)


def case_determinism(lib, mem, n, which=("uniform", "three")):
    """three runs of the same sort into fresh outputs are byte-equal (and right)"""
    if "uniform" in which:
        array_sort(lib, mem, "range", make_keys("uniform", n, 0, 64, seed=5), 0, 64, runs=3)
    if "three" in which:
        array_sort(lib, mem, "pairs", make_keys("three", n, 0, 40, seed=5), 0, 40, runs=3)


# ---- the index sort ----
def index_sort(lib, mem, rec, sizes, seq_base):
    """ani_sort_index over the records `rec` handed over as pieces of `sizes` records"""
    n = len(rec)
    what = "index n=%d pieces=%r" % (n, sizes if len(sizes) < 9 else len(sizes))
    assert sum(sizes) == n
    pieces, o = [], 0
    for s in sizes:
        pieces.append(Buf(mem, rec[o:o + s].copy()))
        o += s
    k = len(sizes)
    piece_ptr = (ctypes.c_void_p * k)(*[p.ptr for p in pieces])
    piece_n = (ctypes.c_size_t * k)(*sizes)
    outs = [out_buf(mem, n, t, 21 + j) for j, t in enumerate((np.uint32, np.int32, np.int32, np.uint32, np.uint64, np.uint32, np.uint64))]
    m_hash, m_seq, m_wpos, tmp_k, tmp_v, s_hash, s_sw = outs

    def call(tmp, tmp_bytes):
        return lib.ani_sort_index(piece_ptr, piece_n, k, seq_base, n, m_hash.ptr, m_seq.ptr, m_wpos.ptr, tmp_k.ptr, tmp_v.ptr, s_hash.ptr, s_sw.ptr,
                                  tmp, ctypes.byref(tmp_bytes), None, None, None)

    tmp_bytes = ctypes.c_size_t(0)
    assert call(None, tmp_bytes) == 0, what
    assert tmp_bytes.value > 0, what
    assert all(b.unchanged() for b in outs), "%s: the size query wrote to an output" % what
    ws = Workspace(mem, tmp_bytes.value)
    rc = call(ws.ptr, tmp_bytes)
    assert rc == 0, "%s: returned %d" % (what, rc)
    seq = rec[:, 1] - np.uint32(seq_base)
    order = np.argsort(rec[:, 0], kind="stable")
    sw = (seq.astype(np.uint64) << np.uint64(32)) | rec[:, 2]
    check_out(m_hash, n, rec[:, 0], what + " mHash")
    check_out(m_seq, n, seq.astype(np.int32), what + " mSeq")
    check_out(m_wpos, n, rec[:, 2].astype(np.int32), what + " mWpos")
    check_out(s_hash, n, rec[order, 0], what + " sHash")
    check_out(s_sw, n, sw[order], what + " sSW")
    for b, name in ((tmp_k, "tmpK"), (tmp_v, "tmpV")):          # scratch: any content, but only n elements of it
        assert np.array_equal(b.get()[n:], b.init[n:]), "%s: written behind the %d-th element of %s" % (what, n, name)
    ws.check_fences(what)
    assert all(p.unchanged() for p in pieces), "%s: a piece was written" % what


def case_index(lib, mem, n, dist, seq_base=1000):
    index_sort(lib, mem, make_records(dist, n, seq_base), split_pieces(n), seq_base)


# ---- argument handling (sort_device.hip) ----
def case_arguments_clamped(lib, mem, n=WAVE + 1):
    """endBit beyond the key is 64, a negative beginBit is 0, endBit <= beginBit is one bit at beginBit"""
    for (begin, end), norm in (((0, 70), (0, 64)), ((31, 70), (31, 64)), ((-3, 9), (0, 9)), ((5, 5), (5, 6)), ((5, 2), (5, 6)), ((-1, -1), (0, 1)),
                               ((63, 0), (63, 64))):
        array_sort(lib, mem, "range", make_keys("uniform", n, *norm, seed=7), begin, end, norm=norm)
    for entry in ("bits", "pairs"):
        array_sort(lib, mem, entry, make_keys("uniform", n, 0, 64, seed=7), 0, 70, norm=(0, 64))
        array_sort(lib, mem, entry, make_keys("uniform", n, 0, 1, seed=7), 0, 0, norm=(0, 1))
        array_sort(lib, mem, entry, make_keys("uniform", n, 0, 1, seed=7), 0, -4, norm=(0, 1))


def _refused(lib, mem, entry, n_claimed, begin, end, expect, short_by=0):
    """a call that must return `expect` and write nothing: buffers of GUARD elements, which a refused call never reaches; no buffers at
    all where n_claimed is more than they hold"""
    k_in, k_out = Buf(mem, pattern(GUARD, np.uint64, 31)), out_buf(mem, 0, np.uint64, 32)
    v_in, v_out = Buf(mem, pattern(GUARD, np.uint32, 33)), out_buf(mem, 0, np.uint32, 34)

    ki, ko, vi, vo = [b.ptr if n_claimed <= GUARD else None for b in (k_in, k_out, v_in, v_out)]

    def call(n, tmp, tmp_bytes):
        if entry == "range":
            return lib.ani_sort_keys_u64_range(ki, ko, n, begin, end, tmp, ctypes.byref(tmp_bytes), None, 0)
        if entry == "bits":
            return lib.ani_sort_keys_u64_bits(ki, ko, n, end, tmp, ctypes.byref(tmp_bytes), None)
        return lib.ani_sort_pairs_u64_u32(ki, ko, vi, vo, n, end, tmp, ctypes.byref(tmp_bytes), None)

    what = "%s n=%d bits [%d, %d)" % (entry, n_claimed, begin, end)
    tmp_bytes = ctypes.c_size_t(0)
    if expect != ERR_BEGIN_BIT:                          # (a range that is refused has no workspace size either)
        assert call(n_claimed, None, tmp_bytes) == 0, what
        assert tmp_bytes.value > 0, what
    else:
        assert call(n_claimed, None, tmp_bytes) == expect, what
    ws = Workspace(mem, 1 << 16)                         # a dummy: the call returns before any device work
    tmp_bytes = ctypes.c_size_t(max(tmp_bytes.value, 1) - short_by)
    rc = call(n_claimed, ws.ptr, tmp_bytes)
    assert rc == expect, "%s: returned %d, not %d" % (what, rc, expect)
    assert ws.all.unchanged() and all(b.unchanged() for b in (k_in, k_out, v_in, v_out)), "%s: a refused call wrote something" % what


def case_arguments_refused(lib, mem):
    for entry in ("range", "bits", "pairs"):
        _refused(lib, mem, entry, 0, 0, 64, 0)                              # n = 0: nothing to do, nothing written
        _refused(lib, mem, entry, GUARD, 0, 64, ERR_WORKSPACE, short_by=1)  # (the size of GUARD keys fits the dummy workspace)
        _refused(lib, mem, entry, 1 << 32, 0, 64, ERR_SIZE)
    for begin, end in ((64, 64), (64, 70), (70, 3), (1 << 20, 0)):
        _refused(lib, mem, "range", GUARD, begin, end, ERR_BEGIN_BIT)


def case_index_arguments(lib, mem):
    """n = 0, a workspace one byte short, n = 2^31 and more pieces than tile counters are refused before any device work; 1020 pieces,
    the most there is room for, are sorted"""
    seq_base = 9
    rec = make_records("min24", 3, seq_base)
    most = [0] * 500 + [2] + [0] * 518 + [1]
    assert len(most) == 1020
    index_sort(lib, mem, rec, most, seq_base)
    piece = Buf(mem, rec)
    outs = [out_buf(mem, 3, t, 41 + j) for j, t in enumerate((np.uint32, np.int32, np.int32, np.uint32, np.uint64, np.uint32, np.uint64))]
    ws = Workspace(mem, 1 << 16)
    for n_pieces, n, short_by, expect in ((1, 0, 0, 0), (1, 3, 1, ERR_WORKSPACE), (1, 1 << 31, 0, ERR_SIZE), (1021, 3, 0, ERR_PIECES)):
        piece_ptr = (ctypes.c_void_p * n_pieces)(*[piece.ptr if n <= 3 else None] * n_pieces)
        piece_n = (ctypes.c_size_t * n_pieces)(*([3] + [0] * (n_pieces - 1)))
        tmp_bytes = ctypes.c_size_t(0)
        args = [piece_ptr, piece_n, n_pieces, seq_base, n] + [b.ptr if n <= 3 else None for b in outs]   # (no buffers where n is more than they hold)
        assert lib.ani_sort_index(*args, None, ctypes.byref(tmp_bytes), None, None, None) == 0
        assert tmp_bytes.value > 0
        tmp_bytes = ctypes.c_size_t(tmp_bytes.value - short_by)
        rc = lib.ani_sort_index(*args, ws.ptr, ctypes.byref(tmp_bytes), None, None, None)
        assert rc == expect, "index n=%d pieces=%d: returned %d, not %d" % (n, n_pieces, rc, expect)
        assert ws.all.unchanged() and piece.unchanged() and all(b.unchanged() for b in outs), "index n=%d pieces=%d: a refused call wrote something" % (
            n, n_pieces)
