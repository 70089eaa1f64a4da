"""Cases for the L2 stage (l2_stage, the second half of map_stage in engine_map.hip, with k_l2_ranges, the length ordering, k_l2_codes,
k_l2_sim<A> / <B>, the collection kernels, the general kernel k_l2 and k_finish_candidates behind it) on SYNTHETIC index records and
SYNTHETIC fragment sketches, shared by the GPU tests (-m gpu, product library) and the CPU-emulation tests (not gpu): test_l2.py.

The sequence-based tests see L2 through mappings and rows, with sketch sizes, range lengths and hash values as murmur makes them.  Here
the records (RecordSet / Index of index_cases.py) and the sketches (Frags of l1_cases.py) are written by hand so that they sit ON the
borders of the fast path: s = 255 / 256 / 319 / 320, ranges of 16384 / 16385 entries, a gap counter at 127 / 128, a first
super-window of one entry, a window that never fits, sketch and reference hashes 0 and 0xffffffff, rank-table buckets with 3 and more
sketch hashes, 40 / 41 candidates of one fragment, event streams of 1728 / 1729 events.  The test entry point ani_l2_check
(host/engine.hpp, TEST INFRASTRUCTURE) runs l1_stage and l2_stage once, exactly as map_stage calls them, and copies out the candidates,
the five result arrays of L2 and the increase of the L2 counters.

The definition below is written from the reference — computeL2MappedRegions (computeMap.hpp:418-497), MIIteratorL2::next
(MIIteratorL2.hpp:74-96) and SlideMapper (slidingMap.hpp:112-284) — and not from l2.hpp: at every placement of the super-window the
shared count is computed FROM SCRATCH as |(s smallest of Q u R) n Q n R| over the set R of the placement's hashes, which is what the
reference's ordered map maintains.  The literal incremental form (SlideMap: pivot, UNIQ / CPLD / REV, DEL / UPD / NOOP) is here too and
is held to the from-scratch count on every case of this file by a CPU-only test per family.  nucIdentity comes from the oracle (orc.identity),
never from the library's LUT.  The expected candidates are those of l1_cases.define.  Only the ROUTING (which candidate takes which
kernel) uses the thresholds that the comments of l2.hpp state, as l1_cases.route does for L1.  Nothing here calls the code under test
to learn what to expect.  Every comparison is exact."""
import bisect
import ctypes
import os

import numpy as np

import l1_cases as lc
import orc
from fastani_amd.api import FragmentSet
from index_cases import ERR_ARG, Index, RecordSet, rng, same
from sort_cases import Buf

# kernels/l2.hpp, as its comments state them: the fast path takes s <= 319 and ranges of <= 16384 entries; class A s <= 255, class B
# s <= 319; a gap counter that would pass 127 sends the candidate to k_l2; k_l2_codes fetches 40 descriptors at once, stages streams
# below 1728 events in LDS and ranks through 2048 buckets of 2^rankShift hashes
CLASS_A_MAX_S, FAST_MAX_S, FAST_MAX_ENTRIES, GAP_MAX = 255, 319, 16384, 127
CAND_BATCH, STAGE_EVENTS, RANK_BUCKETS = 40, 1728, 2048
INFO = ("nFrag", "nCand", "l2FastCandidates", "l2SlowCandidates", "l2SlowLimit", "l2SlowDup", "l2SlowOverflow", "l2Steps", "l2WindowEntries",
        "l2QueryHashes", "l2WindowEntriesB", "l2Launches", "l2ChunkHalvings")
PATHS = (None, "general", "classB")


def bind(lib):
    vp = ctypes.c_void_p
    lib.ani_l2_check.argtypes = [vp, vp, ctypes.c_int32, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.ani_l2_check.restype = ctypes.c_int
    return lib


# =====================================================================================================
# the definition
# =====================================================================================================
def walk(wp, start, end, L, cmw):
    """the three searchIndex calls of computeMap.hpp:424-436 over one contig's positions `wp`, and the placements [b, e) of the
    super-window that the loop of :455 evaluates, advanced as MIIteratorL2::next advances -> (beg, end0, last, [(b, e)])"""
    beg = int(np.searchsorted(wp, start, side="left"))
    end0 = int(np.searchsorted(wp, int(wp[beg]) + cmw, side="left"))
    last = int(np.searchsorted(wp, end + L, side="left"))
    out = []
    b, e, pos = beg, end0, int(wp[beg])
    while e < last:
        out.append((b, e))
        d1, d2 = int(wp[b + 1]) - pos, int(wp[e]) - (pos + cmw - 1)    # MIIteratorL2.hpp:84: the smaller distance, either or both ends
        adv = min(d1, d2)
        pos += adv
        if adv == d1:
            b += 1
        if adv == d2:
            e += 1
    return beg, end0, last, out


def shared_from_scratch(Q, hashes):
    """|U n Q n R|, R = the set of `hashes`, U = the s smallest of Q u R"""
    R = np.unique(hashes)
    U = np.union1d(Q, R)[:len(Q)]
    return len(np.intersect1d(U, np.intersect1d(Q, R, assume_unique=True), assume_unique=True))


def widest_gap(Q, hashes):
    """the largest number of distinct non-query hashes of `hashes` between two neighbouring hashes of Q (below the first, above the last),
    as the fast path's gap counters count them: a reference hash 0xffffffff that is not a sketch hash is not counted (l2.hpp, at
    l2_rank_fast: it reads as the sentinel behind the sketch and takes the spare presence bit of field s, not the counter of gap s)"""
    nonq = np.setdiff1d(np.unique(hashes), Q, assume_unique=True)
    nonq = nonq[nonq != 0xffffffff]
    return int(np.bincount(np.searchsorted(Q, nonq)).max()) if len(nonq) else 0


class SlideMap:
    """SlideMapper (slidingMap.hpp) literally: a sorted container of hash -> [in the query, wposR], a pivot on its s-th key"""

    def __init__(self, Q):
        self.keys = [int(h) for h in Q]
        self.val = {h: [True, None] for h in self.keys}
        self.pivot = self.keys[-1]                                     # :128
        self.shared = 0

    def _both(self, h):
        return self.val[h][0] and self.val[h][1] is not None

    def _step(self, d):
        self.pivot = self.keys[bisect.bisect_left(self.keys, self.pivot) + d]

    def insert(self, h, wpos):
        if h not in self.val:                                          # :143
            bisect.insort(self.keys, h)
            self.val[h] = [False, wpos]
            status = "UNIQ"
        else:
            status = "CPLD" if self.val[h][1] is None else "REV"       # :150
            self.val[h][1] = wpos
        if h <= self.pivot:                                            # :231
            if status == "CPLD":
                self.shared += 1
            elif status == "UNIQ":
                if self._both(self.pivot):
                    self.shared -= 1
                self._step(-1)

    def delete(self, h, wpos):
        pivot_case = False
        if self.val[h][1] == wpos:                                     # :178
            if not self.val[h][0]:
                if h == self.pivot:                                    # :183
                    self._step(+1)
                    if self._both(self.pivot):
                        self.shared += 1
                    pivot_case = True
                self.keys.pop(bisect.bisect_left(self.keys, h))
                del self.val[h]
                status = "DEL"
            else:
                self.val[h][1] = None
                status = "UPD"
        else:
            status = "NOOP"
        if not pivot_case and h <= self.pivot:                         # :264
            if status == "UPD":
                self.shared -= 1
            elif status == "DEL":
                self._step(+1)
                if self._both(self.pivot):
                    self.shared += 1


def shared_incremental(Q, hh, wp, beg, end0, places):
    """the shared count at every placement as computeMap.hpp:448-465 maintains it"""
    sm = SlideMap(Q)
    for j in range(beg, end0):
        sm.insert(int(hh[j]), int(wp[j]))
    out = []
    pb, pe = beg, end0
    for b, e in places:
        if pb != b:
            sm.delete(int(hh[pb]), int(wp[pb]))
        if pe != e:
            sm.insert(int(hh[pe]), int(wp[pe]))
        out.append(sm.shared)
        pb, pe = b, e
    return out


def id_bits(best, s, k, identity):
    """the float bits of nucIdentity if the estimate's upper bound reaches the threshold (computeMap.hpp:375-384), else 0"""
    if best <= 0:
        return 0
    nuc, upper = orc.identity(int(best), int(s), int(k))
    return int(np.array([nuc], dtype=np.float32).view(np.uint32)[0]) if upper >= np.float32(identity) else 0


def route(s, entries, fits, gap, path=None):
    """which kernel finishes a candidate, from the comments of l2.hpp: `limit` (general kernel: s or the range beyond the fast path, or
    ANI_TEST_L2_PATH=general), `done` (the window never fits the range: nothing to simulate), `overflow` (a gap counter would pass 127
    in some placement, `gap` = widest_gap: general kernel), class `A` (s <= 255) or `B` (s <= 319, or everything under ANI_TEST_L2_PATH=classB)"""
    if path == "general" or s > FAST_MAX_S or entries > FAST_MAX_ENTRIES:
        return "limit"
    if not fits:
        return "done"
    if gap > GAP_MAX:
        return "overflow"
    return "A" if s <= CLASS_A_MAX_S and path != "classB" else "B"


class One:
    """one candidate by the definition"""


def candidate(Q, hh, wp, start, end, k, L, w, identity, count="scratch"):
    cmw = L - (w - 1) - (k - 1)                                        # computeMap.hpp:428
    c = One()
    c.s = len(Q)
    c.beg, c.end0, c.last, c.places = walk(wp, start, end, L, cmw)
    c.entries, c.steps = c.last - c.beg, len(c.places)
    if count == "scratch":
        c.shared = [shared_from_scratch(Q, hh[b:e]) for b, e in c.places]
    else:
        c.shared = shared_incremental(Q, hh, wp, c.beg, c.end0, c.places)
    c.best, c.first, c.lastpos = 0, 0, 0
    for (b, e), sh in zip(c.places, c.shared):                         # :468-476: strict improvements only
        if sh > c.best:
            c.best, c.first, c.lastpos = sh, int(wp[b]), int(wp[b])
        elif sh == c.best:
            c.lastpos = int(wp[b])
    # placements that reach the final best at another position than the first optimal one: each must move lastPos
    c.ties = sum(1 for (b, e), sh in zip(c.places, c.shared) if sh == c.best and int(wp[b]) != c.first) if c.best > 0 else 0
    c.ref_start = (c.first + c.lastpos) // 2                           # :496
    c.id_bits = id_bits(c.best, c.s, k, identity)
    # what the routing and the cases' own claims need
    if c.s <= FAST_MAX_S and c.entries <= FAST_MAX_ENTRIES:
        c.gaps = [widest_gap(Q, hh[b:e]) for b, e in c.places]
    else:
        c.gaps = []                                                    # routed by size: the gap counters are never asked
    c.gap, c.gap_first = max(c.gaps + [0]), (c.gaps[0] if c.gaps else 0)
    # one event of the fast path's stream per end moved, after the insert that completes the first window
    c.events = 1 + (c.places[-1][1] - c.end0) + (c.places[-1][0] - c.beg) if c.places else 0
    c.first_window = c.end0 - c.beg
    c.twice = sum(1 for b, e in c.places if len(np.unique(hh[b:e])) < e - b) if c.entries < 5000 else None      # placements that hold some hash twice
    c.single = sum(1 for b, e in c.places if e - b == 1)
    return c


class Expect:
    pass


def define(case):
    """what ani_l2_check must return for `case`: the candidates of l1_cases.define, then every candidate by the definition"""
    p = case
    rec = case.rset.chunk(0, len(case.rset.gcs) - 1)[0]
    e1 = lc.define(rec, case.frags, p.k, p.L, p.identity)
    seq = rec[:, 1].astype(np.int64)
    first = np.searchsorted(seq, np.arange(len(case.rset.contig_len) + 1), side="left")
    hh_all, wp_all = rec[:, 0].astype(np.int64), rec[:, 2].astype(np.int64)
    e = Expect()
    e.l1, e.cand = e1, e1.cand
    e.c = []
    for f, sq, start, end in e1.cand:
        lo, hi = int(first[sq]), int(first[sq + 1])
        Q = case.frags.sketches[f].astype(np.int64)
        e.c.append(candidate(Q, hh_all[lo:hi], wp_all[lo:hi], int(start), int(end), p.k, p.L, p.w, p.identity, case.count))
    col = lambda name, dt=np.int32: np.array([getattr(c, name) for c in e.c], dtype=dt)
    e.best, e.first, e.last, e.ref_start, e.id_bits = col("best"), col("first"), col("lastpos"), col("ref_start"), col("id_bits", np.uint32)
    e.positive = e.best > 0
    return e


def counters(e, path=None, chunk=1 << 21):
    """the increase of the L2 counters for the candidates of `e` under ANI_TEST_L2_PATH = `path` and chunks of `chunk` candidates"""
    r = [route(c.s, c.entries, c.steps > 0, c.gap, path) for c in e.c]
    n = lambda *which: sum(1 for x in r if x in which)
    slow = n("limit", "overflow")
    streams = [x in ("A", "B", "overflow") for x in r]
    return dict(nCand=len(e.c), l2FastCandidates=len(e.c) - slow, l2SlowCandidates=slow, l2SlowLimit=n("limit"), l2SlowDup=0,
                l2SlowOverflow=n("overflow"), l2Steps=sum(c.steps for c in e.c), l2WindowEntries=sum(c.entries for c in e.c),
                l2QueryHashes=sum(c.s for c in e.c), l2WindowEntriesB=sum(c.entries for c, x in zip(e.c, r) if x == "B"),
                l2Launches=sum(1 for a in range(0, len(r), chunk) if any(streams[a:a + chunk])), l2ChunkHalvings=0), r


# =====================================================================================================
# a case: records, sketches, geometry; its definition is computed once and kept
# =====================================================================================================
class Case:
    def __init__(self, name, contigs, sketches, k=16, L=3000, w=None, identity=80.0, genome_fragments=None, count="scratch"):
        self.name, self.k, self.L, self.identity, self.count = name, k, L, identity, count
        self.w = w if w is not None else orc.recommended_window(k, L)
        self.rset = RecordSet(contigs)
        self.frags = lc.Frags(sketches, genome_fragments)
        self.exp = None

    def expect(self):
        if self.exp is None:
            self.exp = define(self)
        return self.exp

    def params(self, engine):
        p = engine.params(self.k, self.L)
        assert self.w == p.windowSize or self.w in (12, 48), (self.w, p.windowSize)
        p.windowSize, p.percentageIdentity = self.w, self.identity
        return p


_cases = {}


def kept(key, make):
    """the case `key`, built and defined once for both halves of the module"""
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def even_sketch(r, s, lo=2, hi=1 << 29):
    """s ascending distinct EVEN hashes in [lo, hi): every odd hash is a non-query hash, and every gap but those of width 2 has some"""
    q = set()
    while len(q) < s:
        q.update(int(x) * 2 for x in r.integers((lo + 1) // 2, hi // 2, s - len(q)))
    return np.array(sorted(q), dtype=np.int64)


def gap_hashes(Q, g, n, top=0xffffffff):
    """up to n distinct odd hashes of gap g of the even sketch Q (gap 0: below Q[0], gap s: above Q[-1])"""
    lo = int(Q[g - 1]) + 1 if g > 0 else 1
    hi = int(Q[g]) if g < len(Q) else top
    return list(range(lo, hi, 2)[:n])


class Result:
    pass


def run_l2(ix, frags, path=None, chunk=0):
    """ani_l2_check of the fragment set against chunk `chunk` of the Index under ANI_TEST_L2_PATH = `path` -> Result"""
    e = ix.engine
    lib = bind(e.lib)
    wire = Buf(ix.buf.mem, frags.wire(ix.p))
    fset = FragmentSet.unpack(e, wire.ptr, wire.init.nbytes, keepalive=wire)
    info = (ctypes.c_uint64 * len(INFO))()
    out, words = ctypes.c_void_p(), ctypes.c_size_t()
    had = os.environ.get("ANI_TEST_L2_PATH")
    if path:
        os.environ["ANI_TEST_L2_PATH"] = path                      # read by l2_stage at every call
    elif had is not None:
        del os.environ["ANI_TEST_L2_PATH"]
    try:
        rc = lib.ani_l2_check(e.h, ix.sk.h, chunk, fset.h, info, ctypes.byref(out), ctypes.byref(words))
    finally:
        if had is None:
            os.environ.pop("ANI_TEST_L2_PATH", None)
        else:
            os.environ["ANI_TEST_L2_PATH"] = had
        fset.close()
    assert wire.unchanged(), "the fragment set was written"
    e._chk(rc)
    r = Result()
    r.info = dict(zip(INFO, (int(x) for x in info)))
    nc = r.info["nCand"]
    assert words.value == 9 * nc and r.info["nFrag"] == frags.n, (words.value, r.info)
    a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int32)), shape=(max(words.value, 1),))[:words.value].copy()
    e.lib.ani_free(out)
    a = a.reshape(9, nc)
    r.cand = a[:4].T.copy()
    r.best, r.first, r.last, r.ref_start, r.id_bits = a[4], a[5], a[6], a[7], a[8].view(np.uint32)
    return r


def describe(case, exp, at):
    c = exp.c[at]
    return "candidate %d of %d %r: s = %d, entries %d, first window %d, steps %d, events %d, widest gap %d" % (
        at, len(exp.c), exp.cand[at].tolist(), c.s, c.entries, c.first_window, c.steps, c.events, c.gap)


def hold(case, exp, got, what):
    """the nine arrays of one call = the definition (the position words only where best > 0: computeMap.hpp never writes them otherwise)"""
    same(what + " candidates", got.cand, exp.cand)
    for name, g, x, everywhere in (("l2Best", got.best, exp.best, True), ("idBits", got.id_bits, exp.id_bits, True), ("l2First", got.first, exp.first, False),
                                   ("l2Last", got.last, exp.last, False), ("refStart", got.ref_start, exp.ref_start, False)):
        bad = np.flatnonzero((g != x) & (everywhere | exp.positive))
        if len(bad):
            at = int(bad[0])
            raise AssertionError("%s: %s differs at %d of %d candidates, first: got %d, expected %d (best %d, first %d, last %d); %s" % (
                what, name, len(bad), len(x), g[at], x[at], exp.best[at], exp.first[at], exp.last[at], describe(case, exp, at)))


def check(world, case, engine=None, chunk=1 << 21, paths=PATHS):
    """the case through the fast path, the general kernel and class B: arrays and counters = the definition; fast and general agree on
    every word and on the three sums -> {path: routing}"""
    engine = engine or world.default
    exp = case.expect()
    ix = Index(engine, world.mem, case.params(engine), case.rset)
    got, routes = {}, {}
    try:
        for path in paths:
            what = "%s [%s]" % (case.name, path or "fast")
            got[path] = g = run_l2(ix, case.frags, path)
            hold(case, exp, g, what)
            want, routes[path] = counters(exp, path, chunk)
            have = {key: g.info[key] for key in want}
            assert have == want, "%s: counters %r, expected %r" % (what, {k: v for k, v in have.items() if v != want[k]},
                                                                      {k: v for k, v in want.items() if v != have[k]})
    finally:
        ix.close()
    if None in got and "general" in got:
        a, b = got[None], got["general"]
        for name in ("best", "first", "last", "ref_start", "id_bits"):
            same("%s: fast path and general kernel, %s" % (case.name, name), getattr(a, name), getattr(b, name))
        for key in ("l2Steps", "l2WindowEntries", "l2QueryHashes"):
            assert a.info[key] == b.info[key], (case.name, key, a.info[key], b.info[key])
    return exp, routes


def reached(case, positive=0.9, ties=1, **want):
    """the case's own claims, from the definition alone (no engine): the routing counts on the fast path, the candidates with best == 0
    (`zero`), the share of candidates with best > 0 (`positive`) and `ties`, the number of placements at which first != last: those
    that reach a candidate's final best at another position than its first optimal one, so that lastPos must move; every case has at
    least `ties` of them (a number, or a predicate)"""
    exp = case.expect()
    cnt, r = counters(exp)
    have = dict(A=r.count("A"), B=r.count("B"), done=r.count("done"), limit=r.count("limit"), overflow=r.count("overflow"),
                zero=int((~exp.positive).sum()), n=len(exp.c),
                ties=sum(c.ties for c in exp.c), apart=sum(1 for c in exp.c if c.best > 0 and c.first != c.lastpos))
    want = dict(want, ties=ties if callable(ties) else (lambda v: v >= ties))
    assert (have["ties"] > 0) == (have["apart"] > 0), have
    for key, v in want.items():
        ok = v(have[key]) if callable(v) else have[key] == v
        assert ok, "%s: %s = %r; %r" % (case.name, key, have[key], have)
    if positive is not None:
        assert len(exp.c) > 0 and int(exp.positive.sum()) >= positive * len(exp.c), "%s: best > 0 at %d of %d candidates" % (
            case.name, int(exp.positive.sum()), len(exp.c))
    return have


# =====================================================================================================
# building blocks
# =====================================================================================================
def geometry(k, L, w=None):
    w = w if w is not None else orc.recommended_window(k, L)
    return w, L - (w - 1) - (k - 1)


def cast(h):
    return np.asarray(h, dtype=np.int64).astype(np.uint32)


def scene_hashes(r, Q, n, planted, low_after, per_gap=60, gaps=None):
    """n hashes for the records of one contig: about 40 % occurrences of the `planted` sketch hashes, the rest odd hashes drawn from
    the gaps of Q (`gaps`: which; default all, gap 0 and gap s first) — those of the lower half of the gaps only from record `low_after` on,
    so that the placements before it keep their smallest sketch hashes"""
    s = len(Q)
    gaps = list(range(s + 1)) if gaps is None else list(gaps)
    pool = {g: gap_hashes(Q, g, per_gap) for g in gaps}
    gaps = [g for g in gaps if pool[g]]
    upper = [g for g in gaps if g >= (s + 1) // 2 and g > 0] or [g for g in gaps if g > 0] or gaps
    out = np.zeros(n, dtype=np.int64)
    todo = [0, s] + [g for g in r.permutation(gaps) if g not in (0, s)]         # every gap once, as far as the records go
    todo = [g for g in todo if g in pool and pool[g]]
    for i in range(n):
        if r.integers(0, 100) < 40:
            out[i] = planted[int(r.integers(0, len(planted)))]
            continue
        if i >= low_after and todo:
            g = todo.pop(0)
        else:
            g = upper[int(r.integers(0, len(upper)))]
        out[i] = pool[g][int(r.integers(0, len(pool[g])))]
    return out


# =====================================================================================================
# sketch sizes
# =====================================================================================================
SKETCH_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 252, 253, 254, 255, 256, 257, 316, 317, 318, 319, 320, 321, 1024, 2048)
GEOMETRY_SIZES = (5, 64, 255, 256, 319, 320)                            # at k = 12, L = 1000


def mixed_positions(r, n, cmw, w, L):
    """n positions at mixed gaps, in the manner of positions(..., "mixed") of index_cases.py — single steps, gaps around w / 2, gaps of
    cmw - 2 .. cmw + 1 and gaps beyond the window — but with a share of gaps of 30 .. 200 and only five wide gaps, all below L: the
    contig is several windows long and stays one stretch, whose placements hold between one record and hundreds"""
    kind = r.integers(0, 100, n - 1)
    gaps = np.where(kind < 20, 1, np.where(kind < 65, 1 + r.integers(0, max(2, w), n - 1), r.integers(30, 200, n - 1)))
    at = r.choice(np.arange(20, n - 20), 5, replace=False)
    gaps[at] = [cmw - 2, cmw - 1, cmw, cmw + 1, cmw + 2 + int(r.integers(0, max(1, L - cmw - 3)))]
    return int(r.integers(0, 50)) + np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)


def quiet(wpos, cmw, L):
    """the records of a mixed contig that must carry no sketch hash: those just behind a wide gap (with a hit just in front of the gap
    they would make a run of nearly L, whose range holds a few records) and those of a stretch between two wide gaps that is no longer
    than a window (its ranges would hold no placement at all)"""
    n = len(wpos)
    out = np.zeros(n, dtype=bool)
    wide = np.flatnonzero(np.diff(wpos) >= cmw - 2)
    for a, b in zip(np.concatenate([[0], wide + 1]), np.concatenate([wide, [n - 1]])):
        if wpos[b] - wpos[a] < cmw + 100:
            out[a:b + 1] = True
    for a in wide:
        out[a + 1:] |= wpos[a + 1:] < wpos[a + 1] + (L - cmw) + 5
    return out


def make_sketch_size(s, k=16, L=3000, seed=0):
    w, cmw = geometry(k, L)
    r = rng(211, s, k, L, seed)
    Q = even_sketch(r, s)
    n = 400
    wpos = mixed_positions(r, n, cmw, w, L)
    # about half of Q is planted — up to 150 of its hashes: about 160 of the contig's 400 records carry a sketch hash, and a contig of
    # 400 records cannot hold half of a sketch of 1024 or 2048 (those sizes take the general kernel, where only s itself matters)
    planted = [int(Q[0])] + [int(x) for x in r.choice(Q, min(max(1, s // 2), 150), replace=False)]
    # the second half of the records holds every gap, gap 0 and gap s first; with more gaps than records there, a random choice of them
    hh = scene_hashes(r, Q, n, planted, low_after=n // 2)
    nonq = hh[:n // 2][~np.isin(hh[:n // 2], Q)]
    for j in np.flatnonzero(quiet(wpos, cmw, L) & np.isin(hh, Q)):
        hh[j] = nonq[int(r.integers(0, len(nonq)))]
    contig = (int(wpos[-1]) + 1 + 200, cast(hh), wpos)
    return Case("sketch size %d k=%d L=%d" % (s, k, L), [contig], [cast(Q)], k=k, L=L)


def sketch_size_case(s, k=16, L=3000):
    """the first seed with best > 0 at nine candidates in ten or more and a placement at which first != last, by the definition"""
    for seed in range(20):
        case = make_sketch_size(s, k, L, seed)
        if case.expect().positive.sum() >= 0.9 * len(case.expect().c) > 0 and sum(c.ties for c in case.expect().c) > 0:
            return case
    raise AssertionError("sketch size %d: no seed with best > 0 everywhere" % s)


def case_sketch_size(world, s, k=16, L=3000):
    case = kept(("size", s, k, L), lambda: sketch_size_case(s, k, L))
    want = "A" if s <= 255 else "B" if s <= 319 else "limit"           # A up to 255, B up to 319, general beyond
    have = reached(case, **{want: lambda v: v >= 1})
    assert have[want] + have["done"] == have["n"], have
    Q = case.frags.sketches[0].astype(np.int64)
    hit = set(np.searchsorted(Q, np.setdiff1d(case.rset.rec[:, 0].astype(np.int64), Q)).tolist())
    if s <= 65:                                                       # non-query hashes in every gap, gap 0 and gap s included
        assert hit == set(range(s + 1)), (s, sorted(hit))
    else:                                                             # more gaps than the contig has records for them: gap 0, gap s and a spread
        assert {0, s} <= hit and len(hit) >= 60 and min(hit - {0}) < s // 2 < max(hit - {s}), (s, len(hit))
    exp, routes = check(world, case)
    assert set(routes["classB"]) - {"done"} == ({"B"} if s <= 319 else {"limit"}) and set(routes["general"]) == {"limit"}


# =====================================================================================================
# range length
# =====================================================================================================
RANGE_LENGTHS = (FAST_MAX_ENTRIES - 1, FAST_MAX_ENTRIES, FAST_MAX_ENTRIES + 1)


def make_range_length(entries, L=3000, k=16):
    """a dense contig (one record per position): hits x_1 < ... < x_j less than L apart merge into the candidate [x_1 - L + 1, x_j], whose
    range [beg, last) is the records of [x_1 - L + 1, x_j + L): x_j - x_1 + 2 L - 1 entries"""
    w, cmw = geometry(k, L)
    r = rng(223, entries)
    Q = even_sketch(r, 40)
    span = entries - (2 * L - 1)
    x1 = L + 500
    chain = list(range(x1, x1 + span, L - 100)) + [x1 + span]
    n = x1 + span + L + 700
    pool = np.array([h for g in range(41) for h in gap_hashes(Q, g, 60)], dtype=np.int64)      # at most 60 distinct per gap: no counter is near 127
    hh = pool[r.integers(0, len(pool), n)]
    inside = r.choice(np.arange(x1 + 1, x1 + span), 2500, replace=False)                        # query hashes between the first hit and the last
    hh[inside] = Q[r.integers(0, 40, len(inside))]
    hh[chain] = Q[r.integers(0, 40, len(chain))]
    return Case("range of %d entries" % entries, [(n, cast(hh), np.arange(n, dtype=np.int64))], [cast(Q)], count="incremental")


def case_range_length(world, entries):
    case = kept(("range", entries), lambda: make_range_length(entries))
    exp = case.expect()
    assert [c.entries for c in exp.c] == [entries], [c.entries for c in exp.c]
    reached(case, **({"A": 1} if entries <= FAST_MAX_ENTRIES else {"limit": 1}))               # fast, fast, slow by limit
    check(world, case)


# =====================================================================================================
# gap counters
# =====================================================================================================
GAP_COUNTS = (126, 127, 128)
GAP_WHERE = ("first_window", "later_insert", "duplicate")


def make_gap_counter(count, where, neighbour, L=3000, k=16, g=20, ff=0):
    """records every 5 positions, the candidate's range begins at record 0 (start clamped to 0).  Gap 20 of a sketch of 40 receives
    `count` distinct non-query hashes: all inside the first super-window, or all but one there and the last one as an insert a few
    placements later, while none has left; `duplicate`: count records, but two of them carry one hash.  `neighbour`: the query hash that
    closes the gap, Q[20], is in the window as well (the gap's field is 2 count + 1) or nowhere in the contig (2 count).
    g = 40: the gap above the whole sketch instead (no query hash closes it); `ff`: the last of its hashes — the late one of
    `later_insert` — is 0xffffffff"""
    w, cmw = geometry(k, L)
    r = rng(227, count, GAP_WHERE.index(where), neighbour, g, ff)
    Q = even_sketch(r, 40)
    Q[20] = Q[19] + 4000                                               # a gap of 2000 odd hashes
    Q = np.array(sorted(set(Q.tolist())), dtype=np.int64)
    assert len(Q) == 40 and Q[20] - Q[19] == 4000 and not (neighbour and g == 40)
    n = 1500
    wpos = 10 + 5 * np.arange(n, dtype=np.int64)
    nwin = int(np.searchsorted(wpos, wpos[0] + cmw))                   # records of the first super-window
    others = np.array([h for x in range(41) if x != g for h in gap_hashes(Q, x, 20)], dtype=np.int64)
    hh = others[r.integers(0, len(others), n)]
    qs = [int(x) for i, x in enumerate(Q) if i != g]
    hits = r.choice(np.arange(5, 590), 60, replace=False)              # hits below L - 1: start = 0; the last of them is the candidate's end
    hh[hits] = [qs[int(i)] for i in r.integers(0, len(qs), len(hits))]
    hh[595] = qs[3]                                                    # wpos 2985: the candidate ends here, last = first record at or beyond 2985 + L
    if neighbour:
        hh[40] = Q[g]
    mine = gap_hashes(Q, g, 200)
    distinct = count - 1 if where == "duplicate" else count
    use = [mine[int(i)] for i in r.choice(len(mine), distinct, replace=False)]
    if ff:
        use[-1] = 0xffffffff
    free = [i for i in range(100, nwin - 20) if i not in set(hits.tolist()) and i != 40]
    slots = sorted(int(i) for i in r.choice(free, count, replace=False))
    if where == "later_insert":
        slots[-1] = nwin + 6                                           # enters with the 7th placement; record 100 leaves with the 101st
    hh[slots] = use + ([use[0]] if where == "duplicate" else [])
    return Case("gap counter %d %s neighbour=%d gap=%d ff=%d" % (count, where, neighbour, g, ff), [(int(wpos[-1]) + 300, cast(hh), wpos)], [cast(Q)])


def case_gap_counter(world, count, where, neighbour):
    case = kept(("gap", count, where, neighbour), lambda: make_gap_counter(count, where, neighbour))
    exp = case.expect()
    assert len(exp.c) == 1, exp.cand
    c = exp.c[0]
    distinct = count - 1 if where == "duplicate" else count
    assert c.gap == distinct and c.beg == 0, (c.gap, c.beg)
    assert c.gap_first == (distinct - 1 if where == "later_insert" else distinct), (c.gap_first, where)
    over = 1 if distinct > GAP_MAX else 0
    reached(case, overflow=over, A=1 - over)
    exp, routes = check(world, case)
    assert routes["classB"] == ["overflow" if over else "B"]


TOP_COUNTS = (127, 128, 129)
TOP_WHERE = ("first_window", "later_insert")


def case_gap_counter_top(world, count, where, ff):
    """the gap above the whole sketch, gap s, at 127, 128 and 129 distinct hashes, one of them 0xffffffff or none: the fast path does not
    count a reference-only 0xffffffff (widest_gap), so 128 with it stay on the fast path and 129 with it go to the general kernel;
    every result word is the definition's either way"""
    case = kept(("top", count, where, ff), lambda: make_gap_counter(count, where, 0, g=40, ff=ff))
    exp = case.expect()
    assert len(exp.c) == 1 and exp.c[0].beg == 0, exp.cand
    c = exp.c[0]
    rec = case.rset.rec[:, 0].astype(np.int64)
    above = np.unique(rec[rec > int(case.frags.sketches[0][-1])])
    assert len(above) == count and (0xffffffff in above) == bool(ff), (len(above), ff)
    assert c.gap == count - ff and c.gap_first == (count - 1 if where == "later_insert" else count - ff), (c.gap, c.gap_first)
    over = 1 if count - ff > GAP_MAX else 0
    reached(case, overflow=over, A=1 - over)
    exp, routes = check(world, case)
    assert routes["classB"] == ["overflow" if over else "B"]


# =====================================================================================================
# window shapes
# =====================================================================================================
class Scene:
    """contigs and fragments side by side; fragment i draws its hashes from a space of its own, [i + 1 << 22, i + 2 << 22): even = its
    sketch, odd = non-query hashes that fall into its gaps; hashes of another space lie below or above its whole sketch"""

    def __init__(self, key, k=16, L=3000, w=None):
        self.k, self.L = k, L
        self.w, self.cmw = geometry(k, L, w)
        self.r = rng(229, *key)
        self.contigs, self.sketches, self.space = [], [], 0

    def sketch(self, s):
        self.space += 1
        return even_sketch(self.r, s, self.space << 22, (self.space + 1) << 22)

    def fill(self, Q, n, gaps=None):
        """n non-query hashes over the upper gaps of Q, at most 120 per gap (no counter comes near 127) and distinct as far as they go:
        what repeats inside a window is then what a case plants"""
        s = len(Q)
        pool = np.array([h for g in (gaps or range((s + 1) // 2 + 1, s + 1)) for h in gap_hashes(Q, g, 120, top=int(Q[-1]) + 4000)], dtype=np.int64)
        pool = self.r.permutation(pool)
        return np.concatenate([pool[:n], pool[self.r.integers(0, len(pool), max(0, n - len(pool)))]])

    def contig(self, wpos, hh, tail=0, length=None):
        wpos = np.asarray(wpos, dtype=np.int64)
        self.contigs.append((length if length is not None else (int(wpos[-1]) + 1 + tail if len(wpos) else 1 + tail), cast(hh), wpos))
        return len(self.contigs) - 1

    def frag(self, Q):
        self.sketches.append(cast(Q))
        return len(self.sketches) - 1

    def case(self, name, **kw):
        return Case(name, self.contigs, self.sketches, k=self.k, L=self.L, w=self.w, **kw)


def make_window_shapes(k=16, L=3000):
    sc = Scene((1, k, L), k, L)
    cmw, r = sc.cmw, sc.r
    s = 24                                                              # m = 1: every occurrence of a sketch hash is a hit
    tags = []

    def one(tag, wpos, hit_at, tail=0, length=None, empty_behind=False):
        """a contig with the records `wpos`, sketch hashes at the indices `hit_at` (the smallest ones of a sketch of its own), fillers elsewhere"""
        Q = sc.sketch(s)
        hh = sc.fill(Q, len(wpos))
        for j, i in enumerate(hit_at):
            hh[i] = Q[j % 8]
        sc.contig(wpos, hh, tail, length)
        if empty_behind:
            sc.contig([], [], tail=5)
        sc.frag(Q)
        tags.append(tag)

    step = lambda n, a, d: a + d * np.arange(n, dtype=np.int64)
    # a first super-window of one entry: the record behind the first is cmw (and cmw + 7) away; the range begins at the first (start clamped)
    for d in (cmw, cmw + 7):
        one("first window of one entry", np.concatenate([[40], step(300, 40 + d, 9)]), [0, 5, 30, 200])
    # fewer records in range than one window: end0 == last.  By the contig's end, and by a gap behind the window
    one("never fits, contig ends", step(50, 100, 11), [3, 20], tail=300)
    one("never fits, contig ends on its last record", step(50, 100, 11), [3, 20], tail=0)
    one("never fits, one record", [77], [0])
    one("never fits, gap behind", np.concatenate([step(60, 0, 13), step(100, 60 * 13 + 2 * L + cmw, 13)]), [2, 30])
    # start clamped to 0 (hit at L - 2), exactly 0 (L - 1) and 1 (L), records from position 0 on
    for x in (L - 2, L - 1, L):
        wp = np.unique(np.concatenate([step(900, 0, 7), [x]]))
        one("start from hit at %d" % x, wp, [int(np.searchsorted(wp, x))])
    # end + L beyond the contig's last record but inside the contig; beyond the contig; exactly the contig's length
    for tail, tag in ((2 * L, "end + L inside the contig, beyond its records"), (0, "end + L beyond the contig"), (None, "end + L = contig length")):
        wp = step(700, 3, 8)
        hit = 640
        if tail is None:
            one(tag, wp, [100, 400, hit], length=int(wp[hit]) + L)
        else:
            one(tag, wp, [100, 400, hit], tail=tail)
    # gaps of cmw - 1, cmw, cmw + 1 between neighbours in the middle of a range: both ends move, one moves, the placement empties to one entry
    for d in (cmw - 1, cmw, cmw + 1):
        wp = np.concatenate([step(250, 5, 10), step(250, 5 + 249 * 10 + d, 10), step(200, 5 + 249 * 10 + d + 249 * 10 + d, 10)])
        one("gap of cmw%+d" % (d - cmw), wp, [200, 249, 250, 300, 499, 500, 600])      # hits on both sides of either gap: one range
    # a contig followed by an empty contig; the last contig of the chunk (ends on its last record)
    one("behind it an empty contig", step(500, 0, 9), [100, 300, 420], empty_behind=True)
    one("the last contig", step(500, 0, 9), [100, 300, 499], tail=0)
    case = sc.case("window shapes k=%d L=%d" % (k, L))
    case.tags = tags
    return case


def case_window_shapes(world, k=16, L=3000):
    case = kept(("shapes", k, L), lambda: make_window_shapes(k, L))
    exp = case.expect()
    by = {}
    for (f, sq, a, b), c in zip(exp.cand, exp.c):
        by.setdefault(case.tags[f], []).append((c, int(a), int(b), int(sq)))
    assert all(t in by for t in case.tags), [t for t in case.tags if t not in by]
    assert sum(1 for c, a, b, sq in by["first window of one entry"] if c.first_window == 1 and c.steps > 1) == 2
    for t in by:
        if t.startswith("never fits"):
            assert all(c.steps == 0 and c.end0 == c.last and c.best == 0 and c.id_bits == 0 for c, a, b, sq in by[t]), t
    L = case.L
    assert [a for c, a, b, sq in by["start from hit at %d" % (L - 2)]] == [0] and [a for c, a, b, sq in by["start from hit at %d" % (L - 1)]] == [0]
    assert [a for c, a, b, sq in by["start from hit at %d" % L]] == [1]
    for t in ("end + L inside the contig, beyond its records", "end + L beyond the contig", "end + L = contig length"):
        for c, a, b, sq in by[t][-1:]:
            assert c.last == int((case.rset.rec[:, 1] == sq).sum()) and c.steps > 0, t                # `last` is the contig's end
            assert (b + L > case.rset.contig_len[sq]) == (t == "end + L beyond the contig"), (t, b, case.rset.contig_len[sq])
    assert any(c.single > 0 for c, a, b, sq in by["gap of cmw+1"]) and all(c.single == 0 for c, a, b, sq in by["gap of cmw-1"])
    assert exp.cand[-1][1] == len(case.rset.contig_len) - 1
    have = reached(case, positive=None, done=lambda v: v >= 4, A=lambda v: v >= 12, zero=lambda v: v >= 4, ties=lambda v: v >= 3)
    check(world, case)


# =====================================================================================================
# same hash
# =====================================================================================================
def make_same_hash(k=16, L=3000):
    sc = Scene((2, k, L), k, L)
    cmw, r = sc.cmw, sc.r
    s = 24
    tags = []
    xs = []
    for d in (cmw - 1, cmw, cmw + 1, cmw + 9, cmw + 10):
        for copies in (2, 3):
            for query in (0, 1):
                for where in ("before", "first_window", "later"):
                    if query and where == "before":
                        continue                                       # an occurrence of a sketch hash is a hit: the range begins at or before it
                    Q = sc.sketch(s)
                    wp = 3 + 9 * np.arange(1500, dtype=np.int64)        # the next record is 9 away: near iff the distance is <= cmw + 9
                    hh = sc.fill(Q, len(wp))
                    hits = [450, 520, 700, 900]                        # start = wpos[450] - L + 1: the range begins at record 117 or 118
                    for j, i in enumerate(hits):
                        hh[i] = Q[1 + j]
                    beg = int(np.searchsorted(wp, wp[450] - L + 1))
                    at = dict(before=beg - 2, first_window=beg + 40, later=beg + 500)[where]
                    X = int(Q[0]) if query else int(Q[0]) - 1          # the smallest sketch hash, or a non-query hash below the whole sketch
                    for c in range(copies):
                        i = int(np.searchsorted(wp, wp[at] + c * d))
                        wp[i] = wp[at] + c * d                         # exactly d apart (the neighbours stay in order: d is no multiple of 9 off by more than 8)
                        hh[i] = X
                    assert np.all(np.diff(wp) > 0)
                    sc.contig(wp, hh, tail=50)
                    sc.frag(Q)
                    tags.append((d - cmw, copies, query, where))
                    xs.append(X)
    # a run of 20 records with one hash, once a sketch hash and once not
    for query in (0, 1):
        Q = sc.sketch(s)
        wp = 3 + 9 * np.arange(1200, dtype=np.int64)
        hh = sc.fill(Q, len(wp))
        for j, i in enumerate((450, 520, 700, 900)):
            hh[i] = Q[1 + j]
        hh[600:620] = int(Q[0]) if query else int(Q[0]) - 1
        sc.contig(wp, hh, tail=50)
        sc.frag(Q)
        tags.append(("run", 20, query, "later"))
        xs.append(int(Q[0]) if query else int(Q[0]) - 1)
    case = sc.case("same hash k=%d L=%d" % (k, L))
    case.tags, case.xs = tags, xs
    return case


def case_same_hash(world, k=16, L=3000):
    case = kept(("same", k, L), lambda: make_same_hash(k, L))
    exp = case.expect()
    rec = case.rset.rec
    first = np.searchsorted(rec[:, 1].astype(np.int64), np.arange(len(case.rset.contig_len) + 1), side="left")
    twice = {t: 0 for t in case.tags}                                  # placements that hold the planted hash twice or more often
    for (f, sq, a, b), c in zip(exp.cand, exp.c):
        hh = rec[first[sq]:first[sq + 1], 0].astype(np.int64)
        twice[case.tags[f]] += sum(1 for pb, pe in c.places if (hh[pb:pe] == case.xs[f]).sum() >= 2)
    # the records are 9 apart: two occurrences share a placement up to a distance of cmw + 7, and the index calls them near up to cmw + 9
    for (d, copies, query, where), v in twice.items():
        if d == "run" or d <= 1:
            assert (v > 0) == (not (where == "before" and copies == 2)), ((d, copies, query, where), v)      # (an occurrence before the range is in no placement)
        elif copies == 2:                                              # (a third occurrence follows a record that was moved: its reach differs)
            assert v == 0, ((d, copies, query, where), v)
    reached(case, A=len(exp.c), ties=lambda v: v >= 1)
    check(world, case)


# =====================================================================================================
# rank table
# =====================================================================================================
RANK_WINDOWS = (24, 12, 48)


def rank_shift(w):
    """k_l2_codes' rank table: 2048 buckets of 2^rankShift hashes from 0 (L2Args::rankShift: the table covers [0, 2^(32 - floor(log2 w) + 1)))"""
    lg = int(np.floor(np.log2(w)))
    return 21 - max(0, lg - 1)


def make_rank_table(w, ff_in_sketch, k=16, L=3000):
    sc = Scene((3, w, ff_in_sketch), k, L, w)
    r, sh = sc.r, rank_shift(w)
    B = 1 << sh
    top = B * (RANK_BUCKETS - 1)                                       # the first hash of the last bucket
    edges = [0, 1, top - 1, top, 0xfffffffe, 0xffffffff]
    Q = set()
    for bucket, n in ((5, 3), (9, 4), (700, 9), (RANK_BUCKETS - 2, 3), (RANK_BUCKETS - 1, 4)):      # 3, 4 and 9 sketch hashes in one bucket
        lo = bucket * B
        Q |= set(int(lo + 10 + 16 * j) for j in range(n))
    Q |= {0, top - 1, top, 0xfffffffe if not ff_in_sketch else 0xffffffff}
    Q |= set(int(x) * 2 + 4 * B for x in r.integers(0, 1 << 27, 30))   # and about one per bucket elsewhere
    Q = np.array(sorted(Q), dtype=np.int64)
    # reference hashes below, between, equal to and above the hashes of the full buckets, and the edges whether sketch hashes or not
    near = set()
    for q in Q:
        near |= {int(q) - 1, int(q) + 1, int(q) + 5}
    near = sorted(h for h in near | set(edges) if 0 <= h <= 0xffffffff and h not in set(Q.tolist()))
    n = 700
    wpos = mixed_positions(r, n, sc.cmw, sc.w, L)
    hh = np.zeros(n, dtype=np.int64)
    planted = Q[::2].tolist() + [int(Q[0]), int(Q[-1])] + [h for h in edges if h in set(Q.tolist())]
    for i in range(n):
        hh[i] = planted[int(r.integers(0, len(planted)))] if r.integers(0, 100) < 45 else near[int(r.integers(0, len(near)))]
    low = [i for i in range(n) if hh[i] in (0, 1)]                     # hashes below the whole sketch push its largest out: keep them out of the first third
    for i in low:
        if i < n // 3 and hh[i] == 1:
            hh[i] = near[-1 - int(r.integers(0, 8))]
    mute = quiet(wpos, sc.cmw, L)
    for j in np.flatnonzero(mute & np.isin(hh, Q)):
        hh[j] = near[int(r.integers(0, len(near)))]
    must = near + [h for h in edges if h in set(Q.tolist())]           # every one of them at least once, behind the first third
    at = r.choice(np.flatnonzero(~mute & (np.arange(n) >= n // 3)), len(must), replace=False)
    hh[at] = must
    sc.contig(wpos, hh, tail=100)
    sc.frag(Q)
    case = sc.case("rank table w=%d ff_in_sketch=%d" % (w, ff_in_sketch))
    case.near, case.Q = near, Q
    return case


def case_rank_table(world, w, ff_in_sketch):
    case = kept(("rank", w, ff_in_sketch), lambda: make_rank_table(w, ff_in_sketch))
    Q, sh = case.Q, rank_shift(w)
    per_bucket = np.bincount(np.minimum(Q >> sh, RANK_BUCKETS - 1))
    assert {3, 4, 9} <= set(per_bucket.tolist()) and per_bucket[-1] >= 3, sorted(set(per_bucket.tolist()))
    have = set(case.rset.rec[:, 0].astype(np.int64).tolist())
    assert {0, 1, (RANK_BUCKETS - 1 << sh) - 1, RANK_BUCKETS - 1 << sh, 0xfffffffe, 0xffffffff} <= have
    assert (0xffffffff in set(Q.tolist())) == bool(ff_in_sketch) and set(case.near) <= have
    reached(case, A=lambda v: v >= 1, limit=0, overflow=0)
    check(world, case)


# =====================================================================================================
# many candidates
# =====================================================================================================
MANY = (1, 3, 4, 5, CAND_BATCH - 1, CAND_BATCH, CAND_BATCH + 1, 2 * CAND_BATCH, 2 * CAND_BATCH + 1)
L2_CHUNKS = (1, 13, 64)


def make_many(n_cand, k=16, L=3000):
    """fragment 0 has n_cand candidates: short contigs that each hold m of its hashes; fragments 2 and 4 have 3 and 5, fragments 1 and 3
    none; two genomes of 2 and 3 fragments: the processing order is 0, 2, 1, 3, 4"""
    sc = Scene((4, n_cand, k, L), k, L)
    r = sc.r
    sketches = [sc.sketch(s) for s in (238, 60, 100, 30, 256)]         # m = 2, 1, ..., and one of class B
    m = [lc.min_hits(len(q), k, 80.0) for q in sketches]
    plan = [(0, n_cand), (2, 3), (4, 5)]
    order = [f for f, n in plan for _ in range(n)]
    for f in r.permutation(order):
        Q = sketches[f]
        n = int(r.integers(45, 70))
        wp = int(r.integers(0, 40)) + np.cumsum(r.integers(20, 200, n))
        hh = sc.fill(Q, n)
        a = int(r.integers(15, n - 20))
        for j in range(m[f] + int(r.integers(0, 3))):                  # m hits or a few more, neighbours
            hh[a + j] = Q[int(r.integers(0, len(Q) // 3))]
        sc.contig(wp, hh, tail=int(r.integers(0, 3)) * 40)
    for Q in sketches:
        sc.frag(Q)
    return sc.case("many candidates %d" % n_cand, genome_fragments=[2, 3])


def case_many(world, n_cand):
    case = kept(("many", n_cand), lambda: make_many(n_cand))
    exp = case.expect()
    per = np.bincount(exp.cand[:, 0], minlength=5).tolist()
    assert per == [n_cand, 0, 3, 0, 5], per
    assert exp.cand[:, 0].tolist() == [0] * n_cand + [2] * 3 + [4] * 5     # not the ascending order of the fragments' processing: 0, 2, 1, 3, 4
    reached(case, A=n_cand + 3, B=5)
    check(world, case)
    for ch in L2_CHUNKS:                                               # chunk borders inside a fragment's candidates
        check(world, case, engine=world.engine(ANI_TEST_L2_CHUNK=ch), chunk=ch)


# =====================================================================================================
# stream length
# =====================================================================================================
STREAMS = (7, 8, 9, STAGE_EVENTS - 1, STAGE_EVENTS, STAGE_EVENTS + 1, 4000)


def make_stream(target, k=16, L=3000):
    """records one or two positions apart from position 0 on, sketch hashes at records below L - 1 (start = 0), the last of them at
    `end`; the contig is cut behind the record that gives the stream its length: found by walking the definition, seed after seed"""
    w, cmw = geometry(k, L)
    for seed in range(200):
        r = rng(233, target, seed)
        Q = even_sketch(r, 40)
        n = 9000
        wp = np.cumsum(r.integers(1, 3, n)) - 1
        end_at = int(np.searchsorted(wp, (400 if target < 100 else L - 60 if target < 3000 else L - 3)))
        pool = np.array([h for g in range(21, 41) for h in gap_hashes(Q, g, 30)], dtype=np.int64)
        hh = pool[r.integers(0, len(pool), n)]
        hits = np.unique(np.concatenate([r.choice(end_at, min(end_at, 200), replace=False), [end_at]]))
        hh[hits] = Q[r.integers(0, 40, len(hits))]
        # cutting the contig behind record e leaves the placements up to the last one that ends at e: one walk of the uncut contig
        beg, e0, full, places = walk(wp, 0, int(wp[end_at]), L, cmw)
        for j, (b, e) in enumerate(places):
            ev = 1 + (e - e0) + (b - beg)
            final = j + 1 == len(places) or places[j + 1][1] > e       # the last placement that ends at e
            if final and (ev == target or (target == 4000 and j + 1 == len(places) and 3900 <= ev <= 4100)):
                keep = e + 1
                return Case("stream of %d events" % target, [(int(wp[keep - 1]) + 1, cast(hh[:keep]), wp[:keep])], [cast(Q)])
    raise AssertionError("no contig with a stream of %d events" % target)


def case_stream(world, target):
    case = kept(("stream", target), lambda: make_stream(target))
    exp = case.expect()
    assert len(exp.c) == 1 and (exp.c[0].events == target or (target == 4000 and 3900 <= exp.c[0].events <= 4100)), [c.events for c in exp.c]
    reached(case, A=1)
    check(world, case)


# =====================================================================================================
# the definition's two forms
# =====================================================================================================
def all_cases():
    """every case of this file: (key, maker)"""
    out = [(("size", s, 16, 3000), lambda s=s: sketch_size_case(s)) for s in SKETCH_SIZES]
    out += [(("size", s, 12, 1000), lambda s=s: sketch_size_case(s, 12, 1000)) for s in GEOMETRY_SIZES]
    out += [(("range", n), lambda n=n: make_range_length(n)) for n in RANGE_LENGTHS]
    out += [(("gap", c, wh, nb), lambda c=c, wh=wh, nb=nb: make_gap_counter(c, wh, nb)) for c in GAP_COUNTS for wh in GAP_WHERE for nb in (0, 1)]
    out += [(("top", c, wh, ff), lambda c=c, wh=wh, ff=ff: make_gap_counter(c, wh, 0, g=40, ff=ff)) for c in TOP_COUNTS for wh in TOP_WHERE for ff in (0, 1)]
    out += [(("shapes", k, L), lambda k=k, L=L: make_window_shapes(k, L)) for k, L in ((16, 3000), (12, 1000))]
    out += [(("same", k, L), lambda k=k, L=L: make_same_hash(k, L)) for k, L in ((16, 3000), (12, 1000))]
    out += [(("rank", w, ff), lambda w=w, ff=ff: make_rank_table(w, ff)) for w in RANK_WINDOWS for ff in (0, 1)]
    out += [(("many", n), lambda n=n: make_many(n)) for n in MANY]
    out += [(("stream", t), lambda t=t: make_stream(t)) for t in STREAMS]
    return out


FAMILIES = ("size", "range", "gap", "top", "shapes", "same", "rank", "many", "stream")


def case_definition_forms(family):
    """the literal incremental form of slidingMap.hpp gives the from-scratch count at every placement of every candidate of every case
    of one family (the range-length cases, defined by the incremental form, are held to the from-scratch count at every 37th placement
    and at the first and the last).  Building and defining the family's cases is most of the time this takes; the cases are kept for
    the tests that run them"""
    n_places = n_cand = 0
    mine = [(key, make) for key, make in all_cases() if key[0] == family]
    assert mine, family
    for key, make in mine:
        case = kept(key, make)
        exp = case.expect()
        rec = case.rset.rec
        first = np.searchsorted(rec[:, 1].astype(np.int64), np.arange(len(case.rset.contig_len) + 1), side="left")
        for (f, sq, a, b), c in zip(exp.cand, exp.c):
            lo, hi = int(first[sq]), int(first[sq + 1])
            hh, wp = rec[lo:hi, 0].astype(np.int64), rec[lo:hi, 2].astype(np.int64)
            Q = case.frags.sketches[f].astype(np.int64)
            if case.count == "scratch":
                other = shared_incremental(Q, hh, wp, c.beg, c.end0, c.places)
                assert other == c.shared, (case.name, f, sq, [(i, x, y) for i, (x, y) in enumerate(zip(other, c.shared)) if x != y][:5])
            else:
                for i in sorted(set(range(0, c.steps, 37)) | {c.steps - 1}):
                    assert shared_from_scratch(Q, hh[c.places[i][0]:c.places[i][1]]) == c.shared[i], (case.name, i)
            n_places += c.steps
            n_cand += 1
    assert n_cand >= len(mine) and n_places > 50 * len(mine), (family, n_cand, n_places)


# =====================================================================================================
def case_arguments(world):
    """what ani_l2_check refuses: null arguments, a chunk that does not exist, a fragment set of other parameters"""
    engine = world.default
    case = kept(("size", 5, 16, 3000), lambda: sketch_size_case(5))
    ix = Index(engine, world.mem, case.params(engine), case.rset)
    lib = bind(engine.lib)
    frags = case.frags
    try:
        wire = Buf(world.mem, frags.wire(ix.p))
        fset = FragmentSet.unpack(engine, wire.ptr, wire.init.nbytes, keepalive=wire)
        wire2 = Buf(world.mem, frags.wire(engine.params(16, 1000)))
        fset2 = FragmentSet.unpack(engine, wire2.ptr, wire2.init.nbytes, keepalive=wire2)
        info = (ctypes.c_uint64 * len(INFO))()
        out, words = ctypes.c_void_p(), ctypes.c_size_t()
        o, w = ctypes.byref(out), ctypes.byref(words)
        call = lib.ani_l2_check
        assert call(None, ix.sk.h, 0, fset.h, info, o, w) == ERR_ARG
        assert call(engine.h, None, 0, fset.h, info, o, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, 0, None, info, o, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, 0, fset.h, None, o, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, 0, fset.h, info, None, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, 0, fset.h, info, o, None) == ERR_ARG
        assert call(engine.h, ix.sk.h, 1, fset.h, info, o, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, -1, fset.h, info, o, w) == ERR_ARG
        assert call(engine.h, ix.sk.h, 0, fset2.h, info, o, w) == ERR_ARG
        assert not out.value
        n = len(case.expect().c)
        assert call(engine.h, ix.sk.h, 0, fset.h, info, o, w) == 0 and list(info)[:2] == [1, n] and words.value == 9 * n
        engine.lib.ani_free(out)
        fset.close()
        fset2.close()
    finally:
        ix.close()
