"""Cases for the index build (build_chunk_index in engine_index.hip with the kernels of kernels/index.hpp: k_index_contig_first,
k_index_links, k_table_block_totals / the host carry loop / k_table_scatter, table_probe, k_index_window_links, k_index_mark_dups,
k_index_pos_sample, and k_index_mark_shared behind Sketch.stats()) on SYNTHETIC minimizer records, shared by the GPU tests (-m gpu,
product library) and the CPU-emulation tests (not gpu, tests/emu build): test_index_build.py.

The end-to-end cases feed these kernels hashes that murmur makes of real sequence.  Here the records (hash, seqId, wpos) are written
by hand and handed to ani_sketch_from_records, so that they sit on the kernels' edges: one hash for a whole 2048-entry table block,
every hash in the table's last slot, the hashes 0 and 0xffffffff, same-hash pairs exactly on the near / not-near border, contigs
without a record at the front, in the middle and at the end of the set, sizes around the 8 entries of a thread, the 1024 entries of a
window-link workgroup and the 2048 of a table block.

Every case takes an Engine and `mem`, the (alloc, upload, download) triple of sort_cases.py for the record buffer.  The test entry
points ani_index_check / ani_index_probe_check / ani_index_links_check (host/engine.hpp, TEST INFRASTRUCTURE) copy a chunk's arrays
out and run table_probe and dup_flag / dup_prev / dup_next on the device.

The definitions below are plain numpy / Python written from the comments of index.hpp; nothing here calls the code under test to
learn what to expect.  Every comparison is exact.

Buffer alignment: every array of a chunk comes from the pool, whose allocations are 16-byte aligned, so the product path cannot
hand these kernels a misaligned buffer; their scalar load / store paths are reached at the tails only (n % 4, n % 8), which the
sizes below cover.  (The misaligned form of k_index_window_links runs in tests/kernel_checks/window_links_check.cpp, on the CPU.)"""
import bisect
import ctypes

import numpy as np

from fastani_amd.api import Sketch
from sort_cases import Buf

THREAD_ENTRIES, WIN_BLOCK, WIN_HALO, TABLE_BLOCK = 8, 1024, 768, 2048          # kernels/index.hpp
WIN_MASK, WIN_SHIFT_A, WIN_MORE_BIT, WIN_DUP_BIT = 0x3fff, 14, 1 << 30, 1 << 31
POS_SAMPLE_SHIFT = 8
ERR_ARG = -1                                                                    # include/ani_abi.h
INFO, S_HASH, S_SW, M_WIN, DUP_BITS, DUP_LIST, CONTIG_FIRST, POS_BASE, POS_SAMPLE, TABLE = range(10)
DTYPE = {INFO: np.uint64, S_HASH: np.uint32, S_SW: np.uint64, M_WIN: np.uint32, DUP_BITS: np.uint32, DUP_LIST: np.uint64, CONTIG_FIRST: np.int32,
         POS_BASE: np.uint32, POS_SAMPLE: np.uint32, TABLE: np.uint32}
INFO_FIELDS = ("n", "nUnique", "nDup", "tableSlots", "tableAlloc", "totalPosBins", "nContigs", "c0", "nGenomes", "g0", "winLinks", "bitWords")

SIZES = (0, 1, 7, 8, 9, WIN_BLOCK - 1, WIN_BLOCK, WIN_BLOCK + 1, TABLE_BLOCK - 1, TABLE_BLOCK, TABLE_BLOCK + 1, 3 * TABLE_BLOCK + 5, 20011)
DISTS = ("min_w", "uniform", "top_half", "low", "distinct", "identical", "edge_single", "edge_runs")
RUN_VALUES = ("uniform", "top_half", "low")
COMBOS = ((16, 3000), (16, 1000), (12, 3000), (12, 1000))                       # (k, fragLen): cmw and w vary


def bind(lib):
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    lib.ani_index_check.argtypes = [vp, vp, i32, ctypes.c_int, vp, u64, ctypes.POINTER(u64)]
    lib.ani_index_probe_check.argtypes = [vp, vp, i32, vp, ctypes.c_size_t, vp]
    lib.ani_index_links_check.argtypes = [vp, vp, i32, vp, ctypes.c_size_t, vp]
    for f in (lib.ani_index_check, lib.ani_index_probe_check, lib.ani_index_links_check):
        f.restype = ctypes.c_int
    return lib


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


# =====================================================================================================
# a reference set of records
# =====================================================================================================
class RecordSet:
    """contigs = [(length, hashes, wpos)], genome_contigs = contigs per genome; the records in position order with set-global seqIds"""

    def __init__(self, contigs, genome_contigs=None):
        genome_contigs = [len(contigs)] if genome_contigs is None else list(genome_contigs)
        assert sum(genome_contigs) == len(contigs)
        self.contig_len = np.array([c[0] for c in contigs], dtype=np.int32)
        self.gcs = np.concatenate([[0], np.cumsum(genome_contigs)]).astype(np.int32)
        h = [np.asarray(c[1], dtype=np.uint32) for c in contigs]
        w = [np.asarray(c[2], dtype=np.int64) for c in contigs]
        for c, (hc, wc) in enumerate(zip(h, w)):                 # what ani_sketch_from_records may be given
            assert len(hc) == len(wc) and (len(wc) == 0 or (wc[0] >= 0 and wc[-1] < contigs[c][0] and np.all(np.diff(wc) > 0))), c
        self.rec = np.zeros((sum(len(x) for x in h), 3), dtype=np.uint32)
        if len(self.rec):
            self.rec[:, 0] = np.concatenate(h)
            self.rec[:, 1] = np.concatenate([np.full(len(x), c, dtype=np.uint32) for c, x in enumerate(h)])
            self.rec[:, 2] = np.concatenate(w)

    def chunk(self, g0, g1):
        """(records with chunk-local seqIds, contig lengths) of the genomes [g0, g1)"""
        c0, c1 = int(self.gcs[g0]), int(self.gcs[g1])
        sel = (self.rec[:, 1] >= c0) & (self.rec[:, 1] < c1)
        rec = self.rec[sel].copy()
        rec[:, 1] -= np.uint32(c0)
        return rec, self.contig_len[c0:c1]


def positions(r, m, cmw, w, style="mixed", start=None):
    """m strictly increasing positions: `dense` every position, `sparse` every gap beyond cmw, `mixed` gaps around w / 2 with single
    steps, gaps of cmw - 2 .. cmw + 1 and gaps beyond cmw among them"""
    first = int(r.integers(0, 50)) if start is None else start
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    if style == "dense":
        gaps = np.ones(m - 1, dtype=np.int64)
    elif style == "sparse":
        gaps = cmw + 1 + r.integers(0, cmw, m - 1)
    else:
        typical = max(1, w // 2)
        kind = r.integers(0, 100, m - 1)
        gaps = np.where(kind < 20, 1, np.where(kind < 90, 1 + r.integers(0, 2 * typical, m - 1),
                                               np.where(kind < 97, cmw - 2 + r.integers(0, 4, m - 1), cmw + 1 + r.integers(0, 3 * cmw, m - 1))))
    return first + np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)


def contig(r, hashes, cmw, w, style="mixed", extra=None):
    wpos = positions(r, len(hashes), cmw, w, style)
    tail = int(r.integers(0, 300)) if extra is None else extra
    return (int(wpos[-1]) + 1 + tail if len(wpos) else 1 + tail, hashes, wpos)


def draw_hashes(r, n, dist, w):
    u32 = lambda m: r.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    if dist in ("min_w", "edge_single", "edge_runs"):               # a window minimizer: the smallest of w hashes
        h = np.full(n, 0xffffffff, dtype=np.uint32)
        for _ in range(w):
            np.minimum(h, u32(n), out=h)
        if dist == "edge_single" and n >= 2:
            at = r.choice(n, 2, replace=False)
            h[at[0]], h[at[1]] = 0, 0xffffffff
        if dist == "edge_runs" and n >= 2:
            at = r.permutation(n)
            a, b = max(1, min(n // 2, 11)), max(1, min(n // 3, 13))
            h[at[:a]], h[at[a:a + b]] = 0, 0xffffffff
        return h
    if dist == "uniform":                                           # about three quarters of them land in the table's last slots
        return u32(n)
    if dist == "top_half":                                          # every slot is nSlots - 1: the table grows past nSlots
        return u32(n) | np.uint32(0x80000000)
    if dist == "low":                                               # every slot is 0: p_i = i
        return (u32(n) & np.uint32(0x3ff)) if n < 1024 else r.permutation(np.arange(n, dtype=np.uint32) % np.uint32(1024))
    if dist == "distinct":
        pool = np.unique(u32(2 * n + 8))
        assert len(pool) >= n
        return r.permutation(pool)[:n]
    assert dist == "identical"
    return np.full(n, u32(1)[0], dtype=np.uint32)


def general_set(n, dist, k, w, cmw, seed=0):
    """n records of hash distribution `dist` over contigs with no record at the front, in the middle (two in a row) and at the end, and
    single-record contigs"""
    r = rng(1, n, DISTS.index(dist), k, cmw, seed)
    h = draw_hashes(r, n, dist, w)
    sizes = [0, 0, 1, 0, 0, 0, 1, 0, 0]                             # front, A, single, two empty, B, single, C, end
    rest = n
    for slot in (2, 6):
        sizes[slot] = min(rest, 1)
        rest -= sizes[slot]
    sizes[1] = rest // 3
    sizes[5] = rest // 2 - rest // 3
    sizes[7] = rest - sizes[1] - sizes[5]
    contigs, o = [], 0
    for s in sizes:
        contigs.append(contig(r, h[o:o + s], cmw, w))
        o += s
    return RecordSet(contigs, [2, 4, 3])


# =====================================================================================================
# the definitions
# =====================================================================================================
def bucket_key(h, w):
    """~ 2^32 (1 - (1 - h / 2^32)^w) in 32-bit fixed point: square-and-multiply on the high halves of the products (uint64 arithmetic)"""
    p = np.uint64(0xffffffff) - h.astype(np.uint64)
    res = np.full(len(h), 0xffffffff, dtype=np.uint64)
    e = int(w)
    while e:
        if e & 1:
            res = (res * p) >> np.uint64(32)
        p = (p * p) >> np.uint64(32)
        e >>= 1
    return np.uint64(0xffffffff) - res


def window_links(seq, wpos, first, cmw1):
    """A / B / more of every entry, as defined at the top of tests/kernel_checks/window_links_check.cpp:
        B[e] = e - (first x in [max(cLo, e - cmw1), e] with wpos[x] > wpos[e] - cmw1)
        A[j] = (first x in [j + 1, min(j + 2 + cmw1, cHi)) with wpos[x] >= wpos[j + 1] + cmw1, else that bound) - j   (0 for a contig's last entry)
        more = wpos[j + A[j]] == wpos[j + 1] + cmw1 (inside the contig)
    wpos is strictly increasing inside a contig, so "the first x with" is a searchsorted over the contig's slice, clamped to the range."""
    n = len(seq)
    out = np.zeros(n, dtype=np.uint32)
    for c in range(len(first) - 1):
        lo, hi = int(first[c]), int(first[c + 1])
        if lo == hi:
            continue
        wc = wpos[lo:hi]
        j = np.arange(lo, hi, dtype=np.int64)
        x = np.maximum(lo + np.searchsorted(wc, wc - cmw1, side="right"), np.maximum(lo, j - cmw1))
        assert np.all(x <= j)
        b = j - x
        a = np.zeros(hi - lo, dtype=np.int64)
        more = np.zeros(hi - lo, dtype=bool)
        if hi - lo > 1:
            tgt = wc[1:] + cmw1
            bound = np.minimum(j[:-1] + 2 + cmw1, hi)
            y = np.minimum(lo + np.searchsorted(wc, tgt, side="left"), bound)
            a[:-1] = y - j[:-1]
            inside = y < hi
            more[:-1][inside] = wpos[y[inside]] == tgt[inside]
        out[lo:hi] = (np.minimum(a, WIN_MASK) << WIN_SHIFT_A | np.minimum(b, WIN_MASK)).astype(np.uint32) | np.where(more, np.uint32(WIN_MORE_BIT), np.uint32(0))
    return out


def define(rec, contig_len, k, w, frag_len):
    """every array of the index over the records `rec` (chunk-local seqIds), from the comments of index.hpp"""
    n, n_contigs = len(rec), len(contig_len)
    h, seq, wpos = rec[:, 0], rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    cmw = frag_len - (w - 1) - (k - 1)
    d = dict(n=n, cmw=cmw)
    order = np.argsort(h, kind="stable")
    d["sHash"] = h[order]
    d["sSW"] = ((seq.astype(np.uint64) << np.uint64(32)) | wpos.astype(np.uint64))[order]
    first = np.searchsorted(seq, np.arange(n_contigs + 1), side="left")
    d["contigFirstMin"] = first.astype(np.int32)
    distinct, run_first, run_cnt = np.unique(d["sHash"], return_index=True, return_counts=True)
    d["nUnique"] = len(distinct)
    # same-hash links: consecutive occurrences ia < ib of one hash in one contig, near iff wpos[ib] - wpos[ia] <= cmw + (wpos[ia + 1] - wpos[ia])
    ia, ib = order[:-1], order[1:]
    pair = (d["sHash"][:-1] == d["sHash"][1:]) & (seq[ia] == seq[ib]) if n > 1 else np.zeros(0, dtype=bool)
    ia, ib = ia[pair].astype(np.int64), ib[pair].astype(np.int64)
    assert np.all(ia < ib)
    near = wpos[ib] - wpos[ia] <= cmw + (wpos[ia + 1] - wpos[ia])
    d["pairs"], d["nearPairs"] = int(pair.sum()), int(near.sum())
    ia, ib = ia[near].astype(np.uint64), ib[near].astype(np.uint64)
    d["dupList"] = np.sort(np.concatenate([ia << np.uint64(32) | np.uint64(1 << 31) | ib, ib << np.uint64(32) | ia]))
    linked = np.zeros(n, dtype=bool)
    linked[ia.astype(np.int64)] = linked[ib.astype(np.int64)] = True
    d["linked"] = linked
    bits = np.zeros(32 * ((n + 31) // 32 + 1), dtype=np.uint8)
    bits[:n] = linked
    d["dupBits"] = np.packbits(bits, bitorder="little").view(np.uint32)
    d["prev"], d["next"] = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    d["prev"][ib.astype(np.int64)] = ia.astype(np.int32)
    d["next"][ia.astype(np.int64)] = ib.astype(np.int32)
    # window links (built iff the L2 fast path can run: 1 <= cmw, cmw + 2 <= the 14-bit offset field)
    d["winLinks"] = bool(n and cmw >= 1 and cmw + 2 <= WIN_MASK)
    if d["winLinks"]:
        d["mWin"] = window_links(seq, wpos, first, cmw - 1) | np.where(linked, np.uint32(WIN_DUP_BIT), np.uint32(0))
    # probe table
    u = len(distinct)
    n_slots = min(max(2 * u, 1024), 0x7ffffff0)
    slot = ((bucket_key(distinct, w) * np.uint64(n_slots)) >> np.uint64(32)).astype(np.int64)
    at = np.zeros(u, dtype=np.int64)
    prev = -1
    for i in range(u):
        prev = at[i] = max(int(slot[i]), prev + 1)
    sentinel = max(n_slots, prev + 1)
    table = np.full((sentinel + 2, 3), 0xffffffff, dtype=np.uint32)
    table[at, 0], table[at, 1], table[at, 2] = distinct, run_first, run_cnt
    table[sentinel] = (0xffffffff, n | 1 << 31, 0)
    d["tableSlots"], d["table"], d["slot"], d["at"] = n_slots, table, slot, at
    d["distinct"], d["runFirst"], d["runCnt"] = distinct, run_first, run_cnt
    # sampled positions
    bins = (contig_len.astype(np.int64) >> POS_SAMPLE_SHIFT) + 1
    d["posBase"] = np.concatenate([[0], np.cumsum(bins)]).astype(np.uint32)
    sample = [first[c] + np.searchsorted(wpos[first[c]:first[c + 1]], np.arange(bins[c]) << POS_SAMPLE_SHIFT, side="left") for c in range(n_contigs)]
    d["posSample"] = np.concatenate(sample + [[n]]).astype(np.uint32)
    return d


def probe_list(d, seed=0):
    """every distinct hash, each of them +-1 where that value is absent, 0 and 0xffffffff, 300 random values -> (hashes, first, cnt)"""
    have = {int(x): (int(f), int(c)) for x, f, c in zip(d["distinct"], d["runFirst"], d["runCnt"])}
    want = set(have) | {0, 0xffffffff}
    for x in have:
        want |= {y for y in (x - 1, x + 1) if 0 <= y <= 0xffffffff}
    r = rng(2, d["n"], seed)
    hashes = np.concatenate([np.array(sorted(want), dtype=np.uint32), r.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)])
    hashes = r.permutation(hashes)
    exp = np.array([have.get(int(x), (0, 0)) for x in hashes], dtype=np.uint32).reshape(-1, 2)
    return hashes, exp


# the half-record list read as dup_prev / dup_next of index.hpp read it
def list_prev(lst, j):
    x = bisect.bisect_left(lst, j << 32)
    if x < len(lst) and lst[x] >> 32 == j and not (lst[x] >> 31) & 1:
        return lst[x] & 0x7fffffff
    return -1


def list_next(lst, j):
    x = bisect.bisect_left(lst, j << 32)
    while x < len(lst) and lst[x] >> 32 == j:
        if (lst[x] >> 31) & 1:
            return lst[x] & 0x7fffffff
        x += 1
    return -1


# =====================================================================================================
# a built index and its comparison with the definitions
# =====================================================================================================
class Index:
    """the device sketch of a RecordSet; the record buffer lives as long as the sketch"""

    def __init__(self, engine, mem, p, rset):
        self.engine, self.lib, self.p, self.rset = engine, bind(engine.lib), p, rset
        self.buf = Buf(mem, rset.rec)
        self.sk = Sketch(engine, p, records=(self.buf.ptr, len(rset.rec), rset.contig_len, rset.gcs))

    def close(self):
        self.sk.close()

    def genome_ranges(self):
        first = self.sk.chunks() + [len(self.rset.gcs) - 1]
        return [(first[c], first[c + 1]) for c in range(len(first) - 1)]

    def fetch(self, chunk, what):
        size = ctypes.c_uint64(0)
        self.engine._chk(self.lib.ani_index_check(self.engine.h, self.sk.h, chunk, what, None, 0, ctypes.byref(size)))
        out = np.zeros(size.value // np.dtype(DTYPE[what]).itemsize, dtype=DTYPE[what])
        self.engine._chk(self.lib.ani_index_check(self.engine.h, self.sk.h, chunk, what, out.ctypes.data if out.size else None, out.nbytes, ctypes.byref(size)))
        assert size.value == out.nbytes
        return out

    def info(self, chunk):
        return dict(zip(INFO_FIELDS, (int(x) for x in self.fetch(chunk, INFO))))

    def probe(self, chunk, hashes):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
        out = np.full((len(hashes), 2), 0xdeadbeef, dtype=np.uint32)
        self.engine._chk(self.lib.ani_index_probe_check(self.engine.h, self.sk.h, chunk, hashes.ctypes.data, len(hashes), out.ctypes.data))
        return out

    def links(self, chunk, entries):
        entries = np.ascontiguousarray(entries, dtype=np.uint32)
        out = np.full((len(entries), 3), -7, dtype=np.int32)
        self.engine._chk(self.lib.ani_index_links_check(self.engine.h, self.sk.h, chunk, entries.ctypes.data, len(entries), out.ctypes.data))
        return out


def same(what, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: shape %r, not %r" % (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, the first at %r: got %r, expected %r" % (what, len(bad), got.size, at, got[at], exp[at]))


def check_chunk(ix, chunk, g0, g1, what=""):
    """every array of chunk `chunk` = the definitions over the records of the genomes [g0, g1); -> the definitions"""
    p = ix.p
    rec, clen = ix.rset.chunk(g0, g1)
    d = define(rec, clen, p.kmerSize, p.windowSize, p.fragLen)
    n = d["n"]
    what = "%s chunk %d (n = %d)" % (what, chunk, n)
    info = ix.info(chunk)
    for key, exp in (("n", n), ("nContigs", len(clen)), ("c0", int(ix.rset.gcs[g0])), ("nGenomes", g1 - g0), ("g0", g0), ("nUnique", d["nUnique"]),
                     ("nDup", len(d["dupList"])), ("tableSlots", d["tableSlots"]), ("tableAlloc", len(d["table"])), ("totalPosBins", len(d["posSample"]) - 1),
                     ("winLinks", int(d["winLinks"]))):
        assert info[key] == exp, "%s: %s is %d, expected %d" % (what, key, info[key], exp)
    same(what + " sHash", ix.fetch(chunk, S_HASH), d["sHash"])
    same(what + " sSW", ix.fetch(chunk, S_SW), d["sSW"])
    same(what + " contigFirstMin", ix.fetch(chunk, CONTIG_FIRST), d["contigFirstMin"])
    same(what + " posBase", ix.fetch(chunk, POS_BASE), d["posBase"])
    same(what + " posSample", ix.fetch(chunk, POS_SAMPLE), d["posSample"])
    dup_list = ix.fetch(chunk, DUP_LIST)
    same(what + " dupList", dup_list, d["dupList"])
    same(what + " dupBits", ix.fetch(chunk, DUP_BITS), d["dupBits"])
    if d["winLinks"]:
        m_win = ix.fetch(chunk, M_WIN)
        same(what + " mWin bit 31", m_win >> np.uint32(31), d["mWin"] >> np.uint32(31))
        same(what + " mWin bits 0..30", m_win & np.uint32(0x7fffffff), d["mWin"] & np.uint32(0x7fffffff))
    # the links of every entry: the returned list bisected here, and dup_flag / dup_prev / dup_next on the device
    lst = [int(x) for x in dup_list]
    same(what + " dup_prev over the list", np.array([list_prev(lst, j) for j in range(n)], dtype=np.int32), d["prev"])
    same(what + " dup_next over the list", np.array([list_next(lst, j) for j in range(n)], dtype=np.int32), d["next"])
    got = ix.links(chunk, np.arange(n, dtype=np.uint32))
    same(what + " dup_flag", got[:, 0], d["linked"].astype(np.int32))
    same(what + " dup_prev", got[:, 1], d["prev"])
    same(what + " dup_next", got[:, 2], d["next"])
    # the probe table, slot by slot, and probes of it
    table = ix.fetch(chunk, TABLE).reshape(-1, 3)
    same(what + " table", table, d["table"])
    hashes, exp = probe_list(d)
    same(what + " table_probe", ix.probe(chunk, hashes), exp)
    return d


def check_index(engine, mem, p, rset, chunks=1, what=""):
    ix = Index(engine, mem, p, rset)
    try:
        ranges = ix.genome_ranges()
        assert len(ranges) >= chunks if chunks > 1 else len(ranges) == 1, ranges
        defs = [check_chunk(ix, c, g0, g1, what) for c, (g0, g1) in enumerate(ranges)]
        assert ix.buf.unchanged(), what + ": the records were written"
        return ix, defs
    except BaseException:
        ix.close()
        raise


def geometry(engine, k, frag_len):
    p = engine.params(k, frag_len)
    return p, p.windowSize, frag_len - (p.windowSize - 1) - (k - 1)


# =====================================================================================================
# the cases
# =====================================================================================================
def case_general(engine, mem, n, dist, k=16, frag_len=3000):
    """every size x every hash distribution"""
    p, w, cmw = geometry(engine, k, frag_len)
    ix, (d,) = check_index(engine, mem, p, general_set(n, dist, k, w, cmw), what="general %s" % dist)
    ix.close()
    if dist == "top_half" and n > 1:                                 # what the distribution is there for
        assert np.all(d["slot"] == d["tableSlots"] - 1) and (n < 1024 or d["at"][-1] >= d["tableSlots"])
    if dist == "low":
        assert np.all(d["slot"] == 0) and np.array_equal(d["at"], np.arange(d["nUnique"]))
    if dist == "uniform" and n >= 1024:
        assert len(d["table"]) > d["tableSlots"] + 2                 # the end cluster runs past nSlots
    if dist in ("edge_single", "edge_runs") and n >= 2:
        assert d["distinct"][0] == 0 and d["distinct"][-1] == 0xffffffff
        assert (d["runCnt"][0] > 1) == (d["runCnt"][-1] > 1) == (dist == "edge_runs" and n >= 7)


RUNS_PLAN = (("singles", 7), ("run", 7), ("pad_to", TABLE_BLOCK - 1), ("run", 8), ("run", 9), ("run", 1), ("pad_to", TABLE_BLOCK + 100), ("run", 4100),
             ("singles", 5), ("run", 2047), ("singles", 3), ("run", 2048), ("singles", 1), ("run", 2049))


def runs_multiset(r, values, w):
    """the hash-sorted index laid out by RUNS_PLAN -> (run lengths in hash order, their hashes)"""
    lengths, at = [], 0
    for kind, v in RUNS_PLAN:
        if kind == "run":
            lengths.append(v)
            at += v
        else:
            m = v if kind == "singles" else v - at
            assert m >= 0
            lengths += [1] * m
            at += m
    hashes = np.sort(draw_hashes(r, len(lengths), "distinct", w))
    if values == "top_half":
        hashes = np.unique(hashes | np.uint32(0x80000000))
    elif values == "low":
        hashes = np.arange(len(lengths), dtype=np.uint32) * np.uint32(3)      # small enough for every slot to be 0
    assert len(hashes) == len(lengths)
    return np.array(lengths), hashes


def case_runs(engine, mem, values, k=16, frag_len=3000):
    """runs of one hash of 1, 7, 8, 9, 2047, 2048, 2049 and 4100 entries, placed in the hash-sorted index so that one starts on the last
    entry of a thread's eight, one on the last entry of a table block, one covers a whole table block (no run start in it: the INT32_MIN
    totals, the host's c > 0 guard, the carry across the block) and the last one ends at n"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(3, RUN_VALUES.index(values), k, frag_len)
    lengths, hashes = runs_multiset(r, values, w)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    n = int(starts[-1])
    # the placement, from the plan alone
    run_start = {int(length): int(s) for length, s in zip(lengths, starts[:-1]) if length > 1}
    assert run_start[7] % THREAD_ENTRIES == THREAD_ENTRIES - 1 and run_start[8] % TABLE_BLOCK == TABLE_BLOCK - 1
    assert run_start[4100] < 2 * TABLE_BLOCK and run_start[4100] + 4100 >= 3 * TABLE_BLOCK          # block 2 has no run start
    assert not np.any((starts[:-1] >= 2 * TABLE_BLOCK) & (starts[:-1] < 3 * TABLE_BLOCK))
    assert run_start[2049] + 2049 == n
    h = r.permutation(np.repeat(hashes, lengths))
    cuts = [0, n // 5, n // 5, n // 2, n // 2 + 1, n]                # an empty contig and a single-record contig among them
    contigs = [contig(r, h[a:b], cmw, w) for a, b in zip(cuts[:-1], cuts[1:])]
    ix, (d,) = check_index(engine, mem, p, RecordSet(contigs), what="runs %s" % values)
    ix.close()
    assert np.array_equal(d["runCnt"], lengths) and np.array_equal(d["runFirst"], starts[:-1])
    assert 0 < d["nearPairs"] < d["pairs"]                           # near and not near
    if values == "top_half":
        assert np.all(d["slot"] == d["tableSlots"] - 1)
    if values == "low":
        assert np.all(d["slot"] == 0) and np.array_equal(d["at"], np.arange(len(lengths)))          # p_i = i from slot 0


def case_near_borders(engine, mem, k, frag_len):
    """same-hash pairs exactly on the near / not-near border and one beyond, neighbours (ib = ia + 1), chains of three and four
    occurrences, one hash for a whole contig (dense, mixed and sparse), the same hash at the end of one contig and the start of the next"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(4, k, frag_len)
    fresh = iter(draw_hashes(r, 20000, "distinct", w))
    fill = lambda m: np.array([next(fresh) for _ in range(m)], dtype=np.uint32)
    contigs, expect_links = [], 0
    for gap in (1, 2, w, cmw // 2):                                   # wpos[ib] - wpos[ia] = cmw + gap (linked) and one more (not linked)
        for beyond in (0, 1):
            last = 5 + cmw + gap + beyond
            inner = np.sort(r.choice(np.arange(5 + gap + 1, last), 20, replace=False))
            wpos = np.concatenate([[5, 5 + gap], inner, [last]])
            h = fill(len(wpos))
            h[-1] = h[0]
            contigs.append((last + 1, h, wpos))
            expect_links += 1 - beyond
    # the border where ia + 1 == ib cannot be missed (the pair is near whatever the gap), nor can two entries beyond cmw with nothing between
    h = fill(6)
    h[1] = h[0]
    h[4] = h[3]
    contigs.append((10 * cmw, h, np.array([3, 3 + 5 * cmw, 3 + 5 * cmw + 1, 3 + 5 * cmw + 2, 3 + 5 * cmw + 3, 3 + 6 * cmw])))
    expect_links += 2
    # chains: three and four occurrences in a row, all near; and a chain whose middle step is far
    h = fill(40)
    h[[3, 6, 8]] = h[3]
    h[[10, 11, 15, 30]] = h[10]
    contigs.append((41 + 100, h, np.arange(40) + 17))
    expect_links += 2 + 3
    wpos = np.concatenate([np.arange(30), 10 * cmw + np.arange(30)])
    h = fill(60)
    h[[2, 20, 40, 55]] = h[2]                                        # near, far, near
    contigs.append((int(wpos[-1]) + 1, h, wpos))
    expect_links += 2
    # one hash for a whole contig
    one = fill(3)
    contigs.append(contig(r, np.full(50, one[0]), cmw, w, "dense"))
    contigs.append(contig(r, np.full(300, one[1]), cmw, w, "mixed"))
    contigs.append(contig(r, np.full(9, one[2]), cmw, w, "sparse"))
    expect_links += 49 + 8                                            # (neighbours are near whatever their distance)
    # the same hash as the last entries of one contig and the first of the next: a link inside each contig, none across
    h1, h2 = fill(12), fill(12)
    h1[-2:] = h2[:2] = h1[-1]
    contigs.append((200, h1, np.arange(12) * 3 + 150))
    contigs.append((200, h2, np.arange(12) * 3))
    expect_links += 2
    ix, (d,) = check_index(engine, mem, p, RecordSet(contigs), what="near borders k=%d L=%d" % (k, frag_len))
    ix.close()
    # (the mixed contig's links depend on its random gaps; the rest is counted above)
    mixed = d["contigFirstMin"][len(contigs) - 4], d["contigFirstMin"][len(contigs) - 3]
    outside = [v for v in d["dupList"] if not mixed[0] <= int(v >> np.uint64(32)) < mixed[1]]
    assert len(outside) == 2 * expect_links, (len(outside), expect_links)
    assert 0 < d["nearPairs"] < d["pairs"]


def case_contigs(engine, mem, k=16, frag_len=3000):
    """contigs of 1, 255, 256 and 257 bases, positions on multiples of 256 and one below, contigs without a record at the front, in the
    middle (two in a row) and at the end, single-record contigs"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(5, k, frag_len)
    spec = [(300, []), (1, [0]), (255, [0, 100, 254]), (256, [255]), (257, [255, 256]), (256, []), (1, []), (255, [254]), (256, [0]),
            (2049, [0, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, 1025, 1279, 1536, 1791, 2047, 2048]), (1024, [1023]), (1025, [1024]),
            (513, [5, 300]), (257, [])]
    contigs = [(length, None, np.array(wpos, dtype=np.int64)) for length, wpos in spec]
    contigs.insert(9, contig(r, np.zeros(700, dtype=np.uint32), cmw, w, "mixed", extra=0))     # ends on its last position
    contigs.insert(12, contig(r, np.zeros(256, dtype=np.uint32), cmw, w, "dense", extra=255))
    n = sum(len(c[2]) for c in contigs)
    h = draw_hashes(r, n, "min_w", w)
    h[r.integers(0, n, n // 10)] = h[0]                              # some same-hash pairs across the little contigs
    out, o = [], 0
    for length, _, wpos in contigs:
        out.append((length, h[o:o + len(wpos)], wpos))
        o += len(wpos)
    ix, (d,) = check_index(engine, mem, p, RecordSet(out, [1, 6, 5, len(out) - 12]), what="contigs")
    ix.close()
    lens = [c[0] for c in out]
    assert {1, 255, 256, 257} <= set(lens) and len(out[0][1]) == 0 and len(out[-1][1]) == 0 and len(out[5][1]) == 0 and len(out[6][1]) == 0


def case_window_links(engine, mem, k, frag_len):
    """the device form of k_index_window_links (LDS staging, the halo, the global loads beyond it, the 16-byte loads and stores): dense
    stretches, gaps beyond cmw, contigs of about 1024 and 1024 +- 768 entries and tiny ones between them"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(6, k, frag_len)
    plan = [(WIN_BLOCK - WIN_HALO, "mixed"), (3, "dense"), (WIN_BLOCK - 1, "dense"), (1, "mixed"), (WIN_BLOCK, "mixed"), (WIN_BLOCK + 1, "sparse"),
            (WIN_BLOCK + WIN_HALO, "mixed"), (2, "sparse"), (WIN_BLOCK + WIN_HALO + 1, "dense"), (WIN_HALO - 1, "mixed"), (cmw + 30, "dense"), (5, "mixed")]
    n = sum(m for m, _ in plan)
    h = draw_hashes(r, n, "min_w", w)
    contigs, o = [], 0
    for m, style in plan:
        contigs.append(contig(r, h[o:o + m], cmw, w, style))
        o += m
    ix, _ = check_index(engine, mem, p, RecordSet(contigs), what="window links k=%d L=%d" % (k, frag_len))
    ix.close()


def pair_cap_set(engine, k=16, frag_len=3000):
    """more than three near pairs among other records"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(7, k, frag_len)
    h = draw_hashes(r, 3000, "min_w", w)
    h[r.integers(0, 3000, 900)] = h[:30][r.integers(0, 30, 900)]
    return p, RecordSet([contig(r, h[:1700], cmw, w), contig(r, h[1700:], cmw, w)])


def case_pair_cap(default_engine, capped_engine, mem):
    """ANI_TEST_DUP_PAIR_CAP=3 (the pair list is sized too small and k_index_links runs again) against the default: the same dupList,
    dupBits and mWin, and both as defined"""
    p, rset = pair_cap_set(default_engine)
    got = []
    for e in (default_engine, capped_engine):
        ix, (d,) = check_index(e, mem, p, rset, what="pair cap")
        assert d["nearPairs"] > 3
        got.append([ix.fetch(0, a) for a in (DUP_LIST, DUP_BITS, M_WIN)])
        ix.close()
    for a, b, name in zip(got[0], got[1], ("dupList", "dupBits", "mWin")):
        same("pair cap 3 against the default: " + name, b, a)


CHUNK_GENOME_RECORDS = 500
CHUNKED_MAX_INDEX_MINIMIZERS = 2 * CHUNK_GENOME_RECORDS + 200      # two of the seven genomes per chunk


def case_chunked(engine, mem, k=16, frag_len=3000):
    """seven genomes in three or more index chunks that share hashes, 0 and 0xffffffff among them: every chunk as defined over its own records,
    and the distinct hashes of the whole set (k_index_mark_shared probes the earlier chunks' tables)"""
    p, w, cmw = geometry(engine, k, frag_len)
    r = rng(8, k, frag_len)
    pool = np.concatenate([draw_hashes(r, 400, "min_w", w), [0, 0xffffffff]]).astype(np.uint32)
    contigs, genome_contigs = [], []
    for g in range(7):
        h = np.concatenate([pool[r.integers(0, len(pool), CHUNK_GENOME_RECORDS - 150)], draw_hashes(r, 146, "uniform", w), [0, 0, 0xffffffff, 0xffffffff]])
        h = r.permutation(h.astype(np.uint32))
        if g == 5:
            h = h[(h != 0) & (h != 0xffffffff)]                     # one genome without the two
        cut = len(h) // 3
        contigs += [contig(r, h[:cut], cmw, w), (77, [], []), contig(r, h[cut:], cmw, w)]
        genome_contigs.append(3)
    rset = RecordSet(contigs, genome_contigs)
    ix, defs = check_index(engine, mem, p, rset, chunks=3, what="chunked")
    assert ix.sk.stats()["unique"] == len(np.unique(rset.rec[:, 0]))
    assert sum(d["nUnique"] for d in defs) > len(np.unique(rset.rec[:, 0]))          # the chunks do share hashes
    assert sum(1 for d in defs if d["n"] and d["distinct"][0] == 0 and d["distinct"][-1] == 0xffffffff) >= 3
    ix.close()


def case_arguments(engine, mem):
    """what the test entry points refuse: a chunk that does not exist, an array that does not exist, a buffer too small, an entry beyond n"""
    p, w, cmw = geometry(engine, 16, 3000)
    ix = Index(engine, mem, p, general_set(100, "min_w", 16, w, cmw))
    lib, e, sk = ix.lib, engine.h, ix.sk.h
    size = ctypes.c_uint64(0)
    out = np.zeros(128, dtype=np.uint32)                            # room for the 100 hashes
    one = np.zeros(4, dtype=np.uint32)
    assert lib.ani_index_check(e, sk, 1, S_HASH, None, 0, ctypes.byref(size)) == ERR_ARG
    assert lib.ani_index_check(e, sk, -1, S_HASH, None, 0, ctypes.byref(size)) == ERR_ARG
    assert lib.ani_index_check(e, sk, 0, 10, None, 0, ctypes.byref(size)) == ERR_ARG
    assert lib.ani_index_check(e, sk, 0, S_HASH, None, 0, None) == ERR_ARG
    assert lib.ani_index_check(e, sk, 0, S_HASH, out.ctypes.data, 399, ctypes.byref(size)) == ERR_ARG and not out.any()
    assert lib.ani_index_check(e, sk, 0, S_HASH, out.ctypes.data, 400, ctypes.byref(size)) == 0 and size.value == 400
    assert lib.ani_index_probe_check(e, sk, 1, one.ctypes.data, 1, out.ctypes.data) == ERR_ARG
    assert lib.ani_index_probe_check(e, sk, 0, None, 1, out.ctypes.data) == ERR_ARG
    assert lib.ani_index_links_check(e, sk, 1, one.ctypes.data, 1, out.ctypes.data) == ERR_ARG
    one[0] = 100
    assert lib.ani_index_links_check(e, sk, 0, one.ctypes.data, 1, out.ctypes.data) == ERR_ARG
    ix.close()


def case_not_resident(engine, mem):
    """a streamed set (one resident chunk): a chunk whose index arrays are not on the device is refused"""
    p, w, cmw = geometry(engine, 16, 3000)
    r = rng(9)
    contigs = [contig(r, draw_hashes(r, CHUNK_GENOME_RECORDS, "min_w", w), cmw, w) for _ in range(6)]
    ix = Index(engine, mem, p, RecordSet(contigs, [1] * 6))
    assert ix.sk.residency()["streaming"] and len(ix.sk.chunks()) >= 3
    size = ctypes.c_uint64(0)
    rcs = [ix.lib.ani_index_check(engine.h, ix.sk.h, c, INFO, None, 0, ctypes.byref(size)) for c in range(len(ix.sk.chunks()))]
    assert set(rcs) <= {0, ERR_ARG} and rcs.count(0) <= 1, rcs
    assert ix.sk.stats()["unique"] == len(np.unique(ix.rset.rec[:, 0]))     # builds chunks, evicts others
    ranges = ix.genome_ranges()
    rcs = [ix.lib.ani_index_check(engine.h, ix.sk.h, c, INFO, None, 0, ctypes.byref(size)) for c in range(len(ranges))]
    assert set(rcs) == {0, ERR_ARG} and 1 <= rcs.count(0) <= 2, rcs
    for c, rc in enumerate(rcs):                                     # a chunk that was rebuilt from the kept records
        if rc == 0:
            check_chunk(ix, c, *ranges[c], what="streamed")
    ix.close()
