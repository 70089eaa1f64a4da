"""Cases for the L1 stage (kernels/l1.hpp behind l1_stage, the first half of map_stage in engine_map.hip: processing order, k_l1_probe,
k_l1_tiny, k_l1_list, k_l1<0, 2032>, k_l1<2032, 4080>, k_l1_big_*, the candidate pool's retry loop, the scan, k_l1_order) on SYNTHETIC
index records and SYNTHETIC fragment sketches, shared by the GPU tests (-m gpu, product library) and the CPU-emulation tests (not gpu):
test_l1.py.

The end-to-end cases see L1 only through mappings and rows, on hashes that murmur makes of real sequence.  Here the index records are
written by hand (RecordSet of index_cases.py -> ani_sketch_from_records) and so are the fragment sketches (a wire buffer laid out as
FragWireHeader of engine_sketch.hip says -> ani_fragset_unpack), so that the seed hits sit on L1's edges: runs that span exactly L - 1
and L, a previous run that ends at start, start - 1 and start + 1, start clamped at 0, runs across a contig border, H = m - 1, m, m + 1,
hit counts on every class border.  The test entry point ani_l1_check (host/engine.hpp, TEST INFRASTRUCTURE) runs l1_stage once and
copies out the ordered candidates, fragHits, the probe results and the routing.

The definition below is computeMap.hpp:283-354 in its sequential form, written from the reference and not from l1.hpp; minimumHits
comes from the oracle (orc.min_hits_relaxed), never from the library's LUT.  Nothing here calls the code under test to learn what to
expect.  Every comparison is exact."""
import ctypes
import os
import struct

import numpy as np

import orc
from fastani_amd.api import FragmentSet
from index_cases import ERR_ARG, Index, RecordSet, rng, same
from sort_cases import Buf

ERR_LIMIT = -4                                                             # include/ani_abi.h
TINY_CAP, CAP_SMALL, CAP_MID, SMALL_MAX_S, MAX_S, HASH_CAP = 256, 2032, 4080, 1024, 2048, 4096      # kernels/l1.hpp
FILTER_MIN, BIG_TILE = 300, 16384
UNWRITTEN = 0xffffffff


def bind(lib):
    vp = ctypes.c_void_p
    lib.ani_l1_check.argtypes = [vp, vp, ctypes.c_int32, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.ani_l1_check.restype = ctypes.c_int
    return lib


# =====================================================================================================
# the definition
# =====================================================================================================
_min_hits = {}


def min_hits(s, k, identity):
    """max(1, minimumHits) of a sketch of s hashes (computeMap.hpp:301, :316), from the oracle"""
    key = (int(s), int(k), float(identity))
    if key not in _min_hits:
        _min_hits[key] = max(1, orc.min_hits_relaxed(int(s), int(k), float(identity)))
    return _min_hits[key]


def candidates(hits, m, L):
    """computeL1CandidateRegions (computeMap.hpp:313-354) over the (seqId << 32 | wpos) hits of one fragment -> [[seq, start, end]]"""
    hits = np.sort(np.asarray(hits, dtype=np.uint64))                  # :320 (seqId, then wpos)
    seq, wpos = (hits >> np.uint64(32)).astype(np.int64), (hits & np.uint64(0xffffffff)).astype(np.int64)
    n = len(hits) - m + 1                                              # :324
    out = []
    if n <= 0:
        return out
    valid = (seq[m - 1:] == seq[:n]) & (wpos[m - 1:] - wpos[:n] < L)  # :332
    for i in np.flatnonzero(valid):
        c = [int(seq[i]), max(0, int(wpos[i + m - 1]) - L + 1), int(wpos[i])]      # :335
        if out and out[-1][0] == c[0] and out[-1][2] >= c[1]:          # :342
            out[-1][2] = max(c[2], out[-1][2])                         # :347
        else:
            out.append(c)
    return out


def route(s, H, tiny=True, lds_max=CAP_MID):
    """where k_l1_probe sends a fragment of s hashes and H seed hits (after the H < m rule), as its comments say"""
    if s <= 0:
        return None
    if s > MAX_S or H > lds_max:
        return "big"
    if H > CAP_SMALL or (s > SMALL_MAX_S and not (H <= TINY_CAP and tiny)):
        return "mid"
    if H <= 0:
        return None
    return "tiny" if H <= TINY_CAP and tiny else "small"


class Expect:
    pass


def define(rec, frags, k, L, identity, tiny=True, lds_max=CAP_MID, lut_max_s=None):
    """what l1_stage must produce for the fragment set `frags` (Frags) against the records `rec` (chunk-local seqIds).
    lut_max_s: sketches longer than the LUT the header's maxS asked for get m = 1 (documented behaviour; None: every sketch is covered)"""
    h = rec[:, 0]
    order = np.argsort(h, kind="stable")
    sh = h[order]
    ssw = ((rec[:, 1].astype(np.uint64) << np.uint64(32)) | rec[:, 2].astype(np.uint64))[order]
    e = Expect()
    e.hits = np.zeros(frags.n, dtype=np.int32)
    e.first, e.cnt = np.full(frags.pool_size, UNWRITTEN, dtype=np.uint32), np.full(frags.pool_size, UNWRITTEN, dtype=np.uint32)
    e.routes = dict(tiny=0, small=0, mid=0, big=0)
    e.route_of, e.m_of = [], []
    per = []
    for f, q in enumerate(frags.sketches):
        s = len(q)
        lo, hi = np.searchsorted(sh, q, side="left"), np.searchsorted(sh, q, side="right")
        cnt = (hi - lo).astype(np.uint32)
        first = np.where(cnt > 0, lo, 0).astype(np.uint32)
        o = int(frags.frag_off[f])
        e.first[o:o + s], e.cnt[o:o + s] = first, cnt
        mine = np.concatenate([ssw[a:b] for a, b in zip(lo, hi) if b > a]) if cnt.any() else np.zeros(0, dtype=np.uint64)
        H = len(mine)
        m = min_hits(s, k, identity) if s > 0 and (lut_max_s is None or s <= lut_max_s) else 1
        if s <= MAX_S and 0 < H < m:
            H = 0                                                      # the probe's rule: fewer hits than a candidate needs count as none
        e.hits[f] = H
        r = route(s, H, tiny, lds_max)
        e.route_of.append(r)
        e.m_of.append(m)
        if r:
            e.routes[r] += 1
        per.append(candidates(mine, m, L))
    # candidate order: fragments in processing order (two or more genomes: a stable sort by fragQSeq), a fragment's own as produced
    proc = np.argsort(frags.frag_qseq, kind="stable") if len(frags.genome_fragments) >= 2 else np.arange(frags.n)
    rows = [(f, c[0], c[1], c[2]) for f in proc for c in per[f]]
    e.cand = np.array(rows, dtype=np.int32).reshape(-1, 4)
    e.per = per
    return e


# =====================================================================================================
# a hand-written fragment set
# =====================================================================================================
class Frags:
    """sketches = one ascending array of distinct hashes per fragment; genome_fragments = fragments per genome.  The hash pool holds the
    sketches in a shuffled order with gaps between them, so that only fragOff says where a fragment's hashes are."""

    def __init__(self, sketches, genome_fragments=None, max_s=None, seed=0):
        self.sketches = [np.asarray(q, dtype=np.uint32) for q in sketches]
        for q in self.sketches:
            assert len(q) <= HASH_CAP and (len(q) < 2 or np.all(q[1:] > q[:-1]))
        self.n = len(self.sketches)
        self.genome_fragments = [self.n] if genome_fragments is None else list(genome_fragments)
        assert sum(self.genome_fragments) == self.n
        self.true_max_s = max([len(q) for q in self.sketches] + [0])
        self.max_s = self.true_max_s if max_s is None else max_s
        r = rng(77, self.n, seed)
        self.frag_off = np.zeros(self.n, dtype=np.uint32)
        at = 0
        for f in r.permutation(self.n):
            at += int(r.integers(0, 4))
            self.frag_off[f] = at
            at += len(self.sketches[f])
        self.pool_size = at + 3
        self.pool = r.integers(0, 1 << 32, self.pool_size, dtype=np.uint64).astype(np.uint32)     # the gaps hold hashes nobody owns
        for f, q in enumerate(self.sketches):
            self.pool[self.frag_off[f]:self.frag_off[f] + len(q)] = q
        self.frag_s = np.array([len(q) for q in self.sketches], dtype=np.int32)
        self.frag_genome = np.repeat(np.arange(len(self.genome_fragments)), self.genome_fragments).astype(np.int32)
        self.frag_qseq = np.concatenate([np.arange(g) for g in self.genome_fragments] + [np.zeros(0)]).astype(np.int32)

    def wire(self, p):
        """the packed form: 256-byte header, genome table, fragOff, fragS, fragGenome, fragQSeq, pool, each section 256-byte aligned"""
        al = lambda x: (x + 255) // 256 * 256
        ng, nf = len(self.genome_fragments), self.n
        o_gf = 256
        o_off = al(o_gf + 4 * ng)
        o_s = al(o_off + 4 * nf)
        o_g = al(o_s + 4 * nf)
        o_q = al(o_g + 4 * nf)
        o_pool = al(o_q + 4 * nf)
        total = al(o_pool + 4 * self.pool_size)
        buf = np.zeros(total, dtype=np.uint8)
        head = struct.pack("<8sI3if3i2Q7Q", b"ANIFRAGS", 1, p.kmerSize, p.windowSize, p.fragLen, p.percentageIdentity, nf, ng, self.max_s,
                           int(self.frag_s.sum()), self.pool_size, o_gf, o_off, o_s, o_g, o_q, o_pool, total)
        assert len(head) == 112
        buf[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        for o, a in ((o_gf, np.array(self.genome_fragments, dtype=np.int32)), (o_off, self.frag_off), (o_s, self.frag_s), (o_g, self.frag_genome),
                     (o_q, self.frag_qseq), (o_pool, self.pool)):
            buf[o:o + a.nbytes] = a.view(np.uint8)
        return buf


class Result:
    pass


def run_l1(ix, chunk, frags, p=None, dense=False):
    """ani_l1_check of the fragment set against chunk `chunk` of the Index -> Result; raises AniError as the engine does"""
    e = ix.engine
    lib = bind(e.lib)
    wire = Buf(ix.buf.mem, frags.wire(p or ix.p))
    fset = FragmentSet.unpack(e, wire.ptr, wire.init.nbytes, keepalive=wire)
    info = (ctypes.c_uint64 * 8)()
    out, words = ctypes.c_void_p(), ctypes.c_size_t()
    had = os.environ.get("ANI_TEST_L1_DENSE")
    if dense:
        os.environ["ANI_TEST_L1_DENSE"] = "1"                      # read by l1_stage at every call
    try:
        rc = lib.ani_l1_check(e.h, ix.sk.h, chunk, fset.h, info, ctypes.byref(out), ctypes.byref(words))
    finally:
        if dense:
            if had is None:
                del os.environ["ANI_TEST_L1_DENSE"]
            else:
                os.environ["ANI_TEST_L1_DENSE"] = had
        fset.close()
    assert wire.unchanged(), "the fragment set was written"
    e._chk(rc)
    r = Result()
    nf, nc, npool = int(info[0]), int(info[1]), int(info[2])
    r.routes = dict(tiny=int(info[3]), small=int(info[4]), mid=int(info[5]), big=int(info[6]))
    r.attempts = int(info[7])
    assert words.value == 4 * nc + nf + 2 * npool and nf == frags.n and npool == frags.pool_size
    a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int32)), shape=(max(words.value, 1),))[:words.value].copy()
    e.lib.ani_free(out)
    r.cand = a[:4 * nc].reshape(4, nc).T.copy()
    r.hits = a[4 * nc:4 * nc + nf]
    r.first = a[4 * nc + nf:4 * nc + nf + npool].view(np.uint32)
    r.cnt = a[4 * nc + nf + npool:].view(np.uint32)
    return r


def check(ix, frags, identity, what, chunk=0, rec=None, dense=False, tiny=True, lds_max=CAP_MID, retry=False, lut_max_s=None):
    """one l1_stage call = the definition; -> (Expect, Result)"""
    p = ix.p
    if rec is None:
        rec = ix.rset.chunk(0, len(ix.rset.gcs) - 1)[0]
    exp = define(rec, frags, p.kmerSize, p.fragLen, identity, tiny, lds_max, lut_max_s)
    got = run_l1(ix, chunk, frags, dense=dense)
    same(what + " fragHits", got.hits, exp.hits)
    same(what + " probeCnt", got.cnt, exp.cnt)
    same(what + " probeFirst", got.first, exp.first)
    assert got.routes == exp.routes, "%s: routed %r, expected %r" % (what, got.routes, exp.routes)
    if len(got.cand) != len(exp.cand):
        fg, fe = np.bincount(got.cand[:, 0], minlength=frags.n), np.bincount(exp.cand[:, 0], minlength=frags.n)
        bad = np.flatnonzero(fg != fe)
        raise AssertionError("%s: %d candidates, expected %d; first fragment that differs: %d (s = %d, m = %d, route %s) got %r expected %r" % (
            what, len(got.cand), len(exp.cand), bad[0], frags.frag_s[bad[0]], exp.m_of[bad[0]], exp.route_of[bad[0]],
            got.cand[got.cand[:, 0] == bad[0]][:, 1:].tolist()[:6], exp.per[bad[0]][:6]))
    if not np.array_equal(got.cand, exp.cand):
        at = int(np.argwhere((got.cand != exp.cand).any(axis=1))[0][0])
        f = int(exp.cand[at, 0])
        raise AssertionError("%s: candidate %d of %d (frag, seq, start, end): got %r, expected %r (fragment %d: s = %d, m = %d, route %s)" % (
            what, at, len(exp.cand), got.cand[at].tolist(), exp.cand[at].tolist(), f, frags.frag_s[f], exp.m_of[f], exp.route_of[f]))
    if retry:
        assert got.attempts > 1, "%s: the candidate pool was large enough at once" % what
    elif len(exp.cand) <= 4096:                                        # the pool's floor is 4096 candidates per stripe: these fit whatever their stripes
        assert got.attempts == 1, "%s: %d attempts of the candidate pool" % (what, got.attempts)
    else:
        assert 1 <= got.attempts <= 3, got.attempts
    return exp, got


# =====================================================================================================
# a scene: contigs with hand-placed records, fragments that hit them
# =====================================================================================================
class Scene:
    def __init__(self, engine, k, L, identity, seed):
        self.engine, self.k, self.L, self.identity = engine, k, L, identity
        self.p = engine.params(k, L)
        self.p.percentageIdentity = identity
        self.r = rng(31, k, L, int(identity), seed)
        self.salt, self.drawn, self.edges = int(self.r.integers(0, 1 << 32)), 0, False
        self.contigs = []                                   # [length or None, {wpos: hash}]
        self.sketches = []

    def m(self, s):
        return min_hits(s, self.k, self.identity)

    def fresh(self, n):
        """n hashes that nothing else in the scene uses (a bijection of a counter), 0 and 0xffffffff among the first"""
        out = []
        while len(out) < n:
            i = np.arange(self.drawn, self.drawn + n - len(out), dtype=np.uint64)
            self.drawn += len(i)
            v = (i * np.uint64(0x9E3779B1) + np.uint64(self.salt)) & np.uint64(0xffffffff)
            out += [int(x) for x in v if 0 < x < 0xffffffff]
        if not self.edges and n >= 2:
            out[0], out[1], self.edges = 0, 0xffffffff, True
        return out

    def contig(self, length=None):
        self.contigs.append([length, {}])
        return len(self.contigs) - 1

    def put(self, c, wpos, h):
        assert wpos >= 0 and wpos not in self.contigs[c][1], (c, wpos)
        self.contigs[c][1][int(wpos)] = int(h)

    def frag(self, s, hit_hashes):
        """a fragment of s hashes: the given ones and fillers that the index does not hold"""
        hit_hashes = sorted(set(int(h) for h in hit_hashes))
        assert len(hit_hashes) <= s, (len(hit_hashes), s)
        self.sketches.append(np.array(sorted(hit_hashes + self.fresh(s - len(hit_hashes))), dtype=np.uint32))
        return len(self.sketches) - 1

    def hits(self, s, where, extra=()):
        """a fragment of s hashes with one hash of its own per (contig, wpos) of `where`, and the hashes `extra`"""
        hs = self.fresh(len(where))
        for (c, w), h in zip(where, hs):
            self.put(c, w, h)
        return self.frag(s, list(hs) + list(extra))

    def record_set(self, genome_contigs=None):
        out = []
        for i, (length, recs) in enumerate(self.contigs):
            wpos = np.array(sorted(recs), dtype=np.int64)
            tail = (0, 1, 300)[i % 3]                                  # some contigs end on their last record
            out.append((length if length is not None else (int(wpos[-1]) + 1 + tail if len(wpos) else 1 + tail), np.array([recs[w] for w in wpos], dtype=np.uint32), wpos))
        return RecordSet(out, genome_contigs)

    def index(self, mem, genome_contigs=None):
        return Index(self.engine, mem, self.p, self.record_set(genome_contigs))


def add_pad(sc, pad, spread=1, h=None):
    """one hash with `pad` occurrences, each alone on a contig of its own (`spread` = 1) or `spread` of them per contig more than 2 L apart:
    far-away hits that raise a fragment's hit count without a run among themselves (for m >= 2)"""
    if pad == 0:
        return []
    h = sc.fresh(1)[0] if h is None else h
    c = None
    for i in range(pad):
        if i % spread == 0:
            c = sc.contig()
        sc.put(c, 5 + (i % spread) * (2 * sc.L + 11), h)
    return [h]


def run_rule_fragments(sc, s, extra=()):
    """the edges of the run rule for a sketch of s hashes (m = minimumHits of s), each fragment on contigs of its own"""
    L, r, m = sc.L, sc.r, sc.m(s)
    room = s - len(extra)
    frags = []

    def one(where):
        if len(where) <= room:
            frags.append(sc.hits(s, where, extra))

    def tight(c, a, n):
        return [(c, a + i) for i in range(n)]

    base = lambda: int(r.integers(L, 3 * L))
    # a run that spans exactly L - 1 (valid) and exactly L (not)
    for span in (L - 1, L):
        c, a = sc.contig(), base()
        one(tight(c, a, m - 1) + [(c, a + span)] if m > 1 else [(c, a)])
    # the run's last hit on the next contig
    if m > 1:
        c, c2 = sc.contig(), sc.contig()
        one(tight(c, base(), m - 1) + [(c2, 0)])
        c, c2 = sc.contig(), sc.contig()
        one([(c, base())] + tight(c2, 3, m - 1))
    # start clamped at 0 (the run ends at m - 1, at L - 2), exactly 0 unclamped (L - 1), and 1 (L)
    for last in (m - 1, L - 2, L - 1, L):
        c = sc.contig()
        one(tight(c, last - (m - 1), m))
    # the previous run's end at start + 1, at start, at start - 1 and further: m + 1 hits a .. a + m - 1, a + D
    for D in (L - 2, L - 1, L, L + 1):
        c, a = sc.contig(), base()
        one(tight(c, a, m) + [(c, a + D)])
    # ... and with the first run clamped at 0
    for D in (L - 1, L):
        c = sc.contig()
        one(tight(c, 0, m) + [(c, D)])
    # a chain: every run merges into the one before (end == start each time), then one that does not, then a second chain on the next contig
    step = (L - 1) // m
    if step >= 1 and 3 * m + 6 <= room:
        c, a = sc.contig(), base()
        chain = [(c, a + i * step) for i in range(2 * m + 2)]
        far = chain[-1][1] + L + 1
        c2 = sc.contig()
        one(chain + tight(c, far, m) + [(c2, 7 + i * step) for i in range(m + 1)])
    # H = m - 1, m, m + 1
    for n in (m - 1, m, m + 1):
        c = sc.contig()
        one(tight(c, base(), n))
    # one hash with m + 2 occurrences in reach of each other, and the same beyond reach
    for gap in (max(1, (L - 1) // (m + 1)), L):
        if m + 2 <= 80:
            c, a, h = sc.contig(), base(), sc.fresh(1)[0]
            for i in range(m + 2):
                sc.put(c, a + i * gap, h)
            frags.append(sc.frag(s, [h] + list(extra)))
    # random hits on three contigs within a few L of each other
    for n in (min(room, 3 * m + 5), min(room, 40)):
        cs = [sc.contig() for _ in range(3)]
        seen = set()
        where = []
        while len(where) < n:
            w = int(r.integers(0, 4 * L))
            if r.integers(0, 2):
                w = w // (L // 8) * (L // 8)                           # some on a grid: distances of exactly k L / 8
            cw = (cs[int(r.integers(0, 3))], w)
            if cw not in seen:
                seen.add(cw)
                where.append(cw)
        one(where)
    return frags


FAMILY_80 = (60, 238, 1024, 1100, 2048, 2049, 4096)                     # m = 1, 2, 15, ..., 33, ..., 72 at k = 16
FAMILY_PADDED = (60, 238, 2048)                                         # with thousands of padding hits per fragment: m = 1, 2, 33
FAMILY_GEOMETRY = (60, 238, 1100, 2049)                                # other k and fragLen: m = 1, 2, ... of that k
FAMILY_95 = (20, 238)                                                   # m = 3, 58 at k = 16


def family_scene(engine, k, L, identity, sizes, pad, hitless=0, seed=0, spread=1):
    sc = Scene(engine, k, L, identity, seed)
    half = add_pad(sc, pad // 2, spread)                                # padding contigs in front of the others and behind them
    sc.pad_hash = half[0] if half else None
    marks = []
    for s in sizes:
        a = len(sc.sketches)
        run_rule_fragments(sc, s, half)
        marks.append((s, a, len(sc.sketches)))
    for i in range(hitless):
        sc.frag((0, 1, 5, 300)[i % 4], [])
    if pad:
        add_pad(sc, pad - pad // 2, spread, half[0] if half else None)  # (pad = 1: no first half, the hash is in no fragment; not used)
    return sc, marks


# the paths: name -> (engine settings, padding hits, hitless fragments, dense launch, the class that must be reached)
PATHS = {
    "tiny1": (dict(), 0, 0, False, "tiny"),
    "tiny2": (dict(), 70, 0, False, "tiny"),
    "tiny4": (dict(), 200, 0, False, "tiny"),
    "classS_dense": (dict(ANI_TEST_L1_TINY=0), 0, 0, True, "small"),
    "classS_list": (dict(ANI_TEST_L1_TINY=0), 0, 400, False, "small"),
    "classS_padded": (dict(), 320, 0, False, "small"),
    "classS_filter0": (dict(ANI_TEST_L1_FILTER_MIN=0, ANI_TEST_L1_TINY=0), 40, 0, False, "small"),
    "classS_nofilter": (dict(ANI_TEST_L1_FILTER_MIN=100000), 320, 0, False, "small"),
    "classM": (dict(), 2100, 0, False, "mid"),
    "classM_filter0": (dict(ANI_TEST_L1_FILTER_MIN=0), 2100, 0, False, "mid"),
    "big_all": (dict(ANI_TEST_L1_LDS_MAX=0), 0, 0, False, "big"),
    "big_100": (dict(ANI_TEST_L1_LDS_MAX=100), 90, 0, False, "big"),
}


TINY_WIDTH = {"tiny1": (1, 64), "tiny2": (65, 128), "tiny4": (129, 256)}       # hits per fragment at 1, 2 and 4 keys per lane (wave_sort_regs)


def knobs(env):
    return dict(tiny=str(env.get("ANI_TEST_L1_TINY", 1)) != "0", lds_max=min(int(env.get("ANI_TEST_L1_LDS_MAX", CAP_MID)), CAP_MID))


def case_run_rule(world, path, k=16, L=3000, identity=80.0, sizes=FAMILY_80):
    """the whole run-rule family through one implementation"""
    env, pad, hitless, dense, must = PATHS[path]
    engine = world.engine(**env) if env else world.default
    if pad > 500 and sizes is FAMILY_80:
        sizes = FAMILY_PADDED
    sc, marks = family_scene(engine, k, L, identity, sizes, pad, hitless, spread=7 if pad > 500 else 1)
    ix = sc.index(world.mem)
    try:
        frags = Frags(sc.sketches)
        exp, got = check(ix, frags, identity, "run rule %s k=%d L=%d id=%g" % (path, k, L, identity), dense=dense, **knobs(env))
        assert exp.routes[must] > 0, exp.routes
        assert len(exp.cand) > 0 and (pad > 0 or (exp.hits == 0).any())
        if must != "big":                                              # every sketch that an LDS class may take went where the case wants it
            want = [r for (s, a, b) in marks if s <= MAX_S for r in exp.route_of[a:b] if r]
            assert want and (must in want), (must, set(want))
        if path in TINY_WIDTH:                                         # the register-sort width under test: every sketch size has fragments of it
            lo, hi = TINY_WIDTH[path]
            for s, a, b in marks:
                if s <= MAX_S:
                    assert any(r == "tiny" and lo <= H <= hi for r, H in zip(exp.route_of[a:b], exp.hits[a:b])), (path, s, list(exp.hits[a:b]))
        small, n = exp.routes["small"], frags.n
        if path == "classS_list":                                      # class S is the exception: k_l1_list and the listed launch
            assert 0 < 2 * small < n, (small, n)
        if path == "classS_dense" and sizes is FAMILY_80:              # the same kind of set: the knob alone makes the launch dense
            assert dense and 0 < 2 * small < n, (small, n)
    finally:
        ix.close()


# =====================================================================================================
def case_class_borders(world, tiny):
    """H on every class border x s on every sketch-size border: what each fragment produced and where it went (one call per H, one for all)"""
    env = dict() if tiny else dict(ANI_TEST_L1_TINY=0)
    engine = world.engine(**env) if env else world.default
    Hs = (64, 65, 128, 129, 256, 257, 2032, 2033, 4080, 4081)
    Ss = (1, 1024, 1025, 2048, 2049, 4096)
    sc = Scene(engine, 16, 3000, 80.0, 5)
    hashes = sc.fresh(len(Hs))
    for H, h in zip(Hs, hashes):                                       # one hash with H occurrences: stretches of 90 records 20..60 apart on contigs of their own
        left = H
        while left:
            c, n, at = sc.contig(), min(left, 90), int(sc.r.integers(0, 500))
            for _ in range(n):
                sc.put(c, at, h)
                at += int(sc.r.integers(20, 61))
            left -= n
    groups = []
    for h in hashes:
        groups.append([sc.frag(s, [h]) for s in Ss])
    ix = sc.index(world.mem)
    try:
        for H, g in zip(Hs, groups):
            exp, got = check(ix, Frags([sc.sketches[f] for f in g]), 80.0, "class borders H=%d tiny=%d" % (H, tiny), **knobs(env))
            assert list(exp.hits) == [H] * len(Ss)
            want = ["tiny" if tiny and H <= 256 else "small" if H <= 2032 else "mid" if H <= 4080 else "big",             # s = 1, 1024
                    "tiny" if tiny and H <= 256 else "mid" if H <= 4080 else "big"]                                         # s = 1025, 2048
            assert exp.route_of == [want[0], want[0], want[1], want[1], "big", "big"], (H, exp.route_of)
        exp, got = check(ix, Frags(sc.sketches), 80.0, "class borders, all, tiny=%d" % tiny, **knobs(env))
        assert len(exp.cand) > 0
    finally:
        ix.close()


def filter_tiles(seq, wpos, shift, bits):
    """the two counter indices of a hit in the noise filter (l1_filter_tiles), to PLACE hits: the expectation does not depend on it"""
    M = 0xffffffff
    ha = (seq * 0x9E3779B1 + (wpos >> shift)) & M
    hb = (seq * 0xC2B2AE3D + ((wpos + (1 << (shift - 1))) >> shift)) & M
    ha ^= ha >> 15
    hb ^= hb >> 15
    return ((ha * 0x85EBCA77) & M) >> (32 - bits), ((hb * 0x27D4EB2F) & M) >> (32 - bits)


def case_noise_filter(world, filter_min, k=16, L=3000):
    """m >= 2, H below and above the threshold: pairs at distance L - 1 across a tile border of either tiling, contigs whose counters
    collide (13 bits in class S, 14 in class M), fragments whose every hit is isolated.  filter_min: None (the default 300), 0 (always),
    large (never)"""
    env = dict() if filter_min is None else dict(ANI_TEST_L1_FILTER_MIN=filter_min)
    engine = world.engine(**env) if env else world.default
    sc = Scene(engine, k, L, 80.0, 9)
    shift = 1
    while (1 << shift) < 2 * L:
        shift += 1
    T = 1 << shift
    nc = 400
    cs = [sc.contig(6 * T) for _ in range(nc)]

    def colliding(bits, among):
        """two contigs with a tile each whose counters of the first tiling collide -> ([contig, contig], [(contig, wpos), (contig, wpos)])"""
        idx, found = {}, None
        for c in among:
            for tile in range(4, 6):
                ia, ib = filter_tiles(c, tile * T + 17, shift, bits)
                if ia in idx and idx[ia][0] != c:
                    found = (idx[ia], (c, tile))
                idx[ia] = (c, tile)
        assert found is not None, bits
        assert filter_tiles(found[0][0], found[0][1] * T + 18, shift, bits)[0] == filter_tiles(found[1][0], found[1][1] * T + 18, shift, bits)[0]
        return [c for c, tile in found], [(c, tile * T + 17) for c, tile in found]

    collide, collide_at = colliding(13, cs[60:])                       # class S: 13-bit counters
    collide_m, collide_m_at = colliding(14, [c for c in cs[60:] if c not in collide])      # class M: 14-bit counters
    pad_few, pad_many = add_pad(sc, 270), add_pad(sc, 340)             # H below / above the default threshold
    s2, s15, s_mid = 238, 1024, 1100                                   # s_mid > kL1SmallMaxS: class M whatever the hit count above 256
    assert sc.m(s2) == 2 and sc.m(s15) >= 3 and sc.m(s_mid) >= 3
    pairs = []
    for j, x in enumerate((T - 1, T - (L - 1), T + T // 2 - 1, T + T // 2 - (L - 1), 2 * T - L // 2, 2 * T + T // 2 - L // 2, 3 * T - L, 3 * T + T // 2 - L)):
        pairs.append((x, x + (L - 1 if j < 6 else L)))                 # the last two: distance L, no run
    at, mids = 0, []
    for pi, pad in enumerate((pad_few, pad_many)):
        for x, y in pairs:                                             # m = 2: each pair on a contig of its own ...
            c = cs[at % nc]
            at += 1
            sc.hits(s2, [(c, x), (c, y)], pad)
        # ... all pairs in one fragment, on the two colliding contigs and a third, with isolated hits on the colliding ones
        d = 3 + 50 * pi
        where = [(collide[j % 2], x + d) for j, (x, y) in enumerate(pairs)] + [(collide[j % 2], y + d) for j, (x, y) in enumerate(pairs)]
        where = sorted(set(where)) + [(c, w + pi) for c, w in collide_at]
        sc.hits(s2, where, pad)
        # m = 15: fourteen hits at x .. and the last at distance L - 1 (a run) / L (none), across the tile border
        for x, y in pairs[:2] + pairs[6:]:
            c = cs[at % nc]
            at += 1
            sc.hits(s15, [(c, x + i) for i in range(sc.m(s15) - 1)] + [(c, y)], pad)
        sc.frag(s2, pad)                                               # every hit isolated
        sc.frag(s15, pad)
        # class M (14-bit counters): the same runs of m hits across the tile borders, each on a contig of its own ...
        mm = sc.m(s_mid)
        mid0 = len(sc.sketches)
        for x, y in pairs[:4] + pairs[6:]:
            c = cs[at % nc]
            at += 1
            sc.hits(s_mid, [(c, x + i) for i in range(mm - 1)] + [(c, y)], pad)
        # ... all of them in one fragment on the two contigs whose counters collide, with isolated hits in the colliding tiles
        where = []
        for j, (x, y) in enumerate(pairs):
            where += [(collide_m[j % 2], x + d + i) for i in range(mm - 1)] + [(collide_m[j % 2], y + d)]
        sc.hits(s_mid, sorted(set(where)) + [(c, w + pi) for c, w in collide_m_at], pad)
        sc.frag(s_mid, pad)                                            # every hit isolated
        mids.append((mid0, len(sc.sketches)))
    ix = sc.index(world.mem)
    try:
        exp, got = check(ix, Frags(sc.sketches), 80.0, "noise filter min=%r L=%d" % (filter_min, L), **knobs(env))
        H = exp.hits
        assert (H[H > 0] < FILTER_MIN).any() and (H > FILTER_MIN).any() and exp.routes["small"] > 0
        assert [len(c) for c in exp.per[:6]] == [1] * 6 and [len(c) for c in exp.per[6:8]] == [0, 0]
        for (a, b), below in zip(mids, (True, False)):                 # class M on both sides of the threshold, runs and none
            assert exp.route_of[a:b] == ["mid"] * (b - a), exp.route_of[a:b]
            assert ((H[a:a + 6] < FILTER_MIN) if below else (H[a:b] > FILTER_MIN)).all(), H[a:b]
            assert [len(c) for c in exp.per[a:a + 6]] == [1, 1, 1, 1, 0, 0] and len(exp.per[b - 2]) > 0 and len(exp.per[b - 1]) == 0
    finally:
        ix.close()


def case_big_key_widths(world, b=12, c=4):
    """maxContigLen = 2^b - 1 and 2^b, nContigs = 2^c - 1, 2^c, 2^c + 1: the field widths of the batched path's key"""
    engine = world.engine(ANI_TEST_L1_LDS_MAX=0)
    for length in ((1 << b) - 1, 1 << b):
        for delta in (-1, 0, 1):
            sc = Scene(engine, 16, 3000, 80.0, 100 + delta)
            n = (1 << c) + delta
            cs = [sc.contig(length if i in (0, n - 1) else 1 + i * 37) for i in range(n)]
            for j, s in enumerate((2049, 238, 60)):                    # positions 4 i + j: the first of them on the last base of the last contig
                m = sc.m(s)
                sc.hits(s, [(cs[-1], length - 1 - 4 * i - j) for i in range(m)] + [(cs[0], 4 * i + j) for i in range(m)]
                        + [(cs[n // 2], 4 * i + j) for i in range(min(m, (n // 2) * 9))])
                sc.hits(s, [(cs[i], 3 + 4 * j) for i in range(1, n - 1)] + [(cs[0], length - 1 - j)])
            ix = sc.index(world.mem)
            try:
                exp, got = check(ix, Frags(sc.sketches), 80.0, "big key widths len=%d contigs=%d" % (length, n), tiny=True, lds_max=0)
                assert exp.routes["big"] == len(sc.sketches) and len(exp.cand) > 0
                assert int(ix.rset.contig_len.max()) == length and len(ix.rset.contig_len) == n
            finally:
                ix.close()


def case_big_tiles(world):
    """the tile border of k_l1_big_gather: a fragment whose only hit hash has 16384 occurrences (one tile, exactly full) and one whose
    only hit hash has 16385 (a second tile of one hit); the same two with two more hits of their own (second tiles of 2 and 3 hits);
    s > 2048 with H = 0"""
    engine = world.default
    sc = Scene(engine, 16, 3000, 80.0, 21)
    for H, s in ((BIG_TILE, 60), (BIG_TILE + 1, 238)):                 # m = 1 and m = 2
        h = sc.fresh(1)[0]
        left = H
        while left:
            c, n, at = sc.contig(), min(left, 700), int(sc.r.integers(0, 100))
            for _ in range(n):
                sc.put(c, at, h)
                at += int(sc.r.integers(1, 2600))
            left -= n
        sc.frag(s, [h])                                                # the rest of the sketch: fillers that the index does not hold
        c = sc.contig()
        sc.hits(s, [(c, 10), (c, 10 + sc.L - 1)], [h])
    sc.frag(2049, [])
    ix = sc.index(world.mem)
    try:
        exp, got = check(ix, Frags(sc.sketches), 80.0, "big tiles")
        assert list(exp.hits) == [BIG_TILE, BIG_TILE + 2, BIG_TILE + 1, BIG_TILE + 3, 0] and exp.routes["big"] == 5
        assert all(len(c) > 20 for c in exp.per[:4]) and len(exp.cand) > 100
    finally:
        ix.close()


def case_big_groups(world):
    """the batched path's groups: a border between two big fragments (by hits and by fragment count), one fragment larger than the budget"""
    sc0 = None
    for env in (dict(ANI_TEST_L1_BIG_GROUP_HITS=50), dict(ANI_TEST_L1_BIG_GROUP_FRAGS=3), dict(ANI_TEST_L1_BIG_GROUP_HITS=1, ANI_TEST_L1_BIG_GROUP_FRAGS=2)):
        env = dict(env, ANI_TEST_L1_LDS_MAX=10)
        engine = world.engine(**env)
        sc = Scene(engine, 16, 3000, 80.0, 33)
        pad = add_pad(sc, 20)
        run_rule_fragments(sc, 60, pad)                                # 21 .. 60 hits each: a group holds one or two
        run_rule_fragments(sc, 2049)
        sc.sketches = sc.sketches[::5]
        c = sc.contig()
        sc.hits(238, [(c, 5 + 11 * i) for i in range(120)], pad)       # larger than the budget of 50 on its own
        sc.frag(4096, [])
        ix = sc.index(world.mem)
        try:
            exp, got = check(ix, Frags(sc.sketches), 80.0, "big groups %r" % (env,), **knobs(env))
            assert exp.routes["big"] >= 8 and exp.hits.max() > 50 and len(exp.cand) > 0
        finally:
            ix.close()


def case_launch_shape(world, n_frag, mostly_small):
    """nFrag around kL1ProbeFrags, kL1TinyFrags and the workgroup size; class S as the rule (dense launch) or as the exception (the list
    launch, with hitless fragments and s = 0 fragments among the others)"""
    engine = world.engine(ANI_TEST_L1_TINY=0)
    sc = Scene(engine, 16, 3000, 80.0, n_frag * 2 + mostly_small)
    c = sc.contig()
    at = 0
    for f in range(n_frag):
        kind = f % 8
        hit = kind != 3 if mostly_small else kind in (1, 6)
        if n_frag == 1:
            hit = True
        if hit:
            s = (60, 238)[f % 2]
            m = sc.m(s)
            sc.hits(s, [(c, at + i * 5) for i in range(m + f % 3)])
            at += 4 * sc.L if f % 5 else sc.L - 1 - 5 * (m - 1)        # now and then in reach of the next fragment's hits: of no concern to either
        else:
            sc.frag((0, 7, 0, 60)[f % 4], [])
    ix = sc.index(world.mem)
    try:
        exp, got = check(ix, Frags(sc.sketches), 80.0, "launch shape nFrag=%d small=%d" % (n_frag, mostly_small), tiny=False)
        assert (2 * exp.routes["small"] >= n_frag) == bool(mostly_small) and exp.routes["small"] > 0
    finally:
        ix.close()


def case_genomes(world, genome_fragments):
    """two and three genomes of unequal fragment counts: the processing order is a stable sort of the fragments by fragQSeq"""
    for env in (dict(), dict(ANI_TEST_L1_TINY=0)):
        engine = world.engine(**env) if env else world.default
        sc = Scene(engine, 16, 3000, 80.0, len(genome_fragments))
        n = sum(genome_fragments)
        c = sc.contig()
        for f in range(n):
            if f % 4 == 2:
                sc.frag(30, [])
            else:
                sc.hits(60, [(c, f * 40 + i * 5 * sc.L) for i in range(1 + f % 3)])      # m = 1: one to three candidates each
        ix = sc.index(world.mem)
        try:
            frags = Frags(sc.sketches, genome_fragments)
            exp, got = check(ix, frags, 80.0, "genomes %r %r" % (genome_fragments, env), **knobs(env))
            order = exp.cand[:, 0]
            assert len(order) > n // 2 and not np.all(np.diff(order) >= 0)             # not the ascending order
        finally:
            ix.close()


def case_pool_retry(world):
    """ANI_TEST_CAND_POOL_MIN=1: the first candidate pool is too small, the class launches run again, the candidates are the same"""
    engine = world.engine(ANI_TEST_CAND_POOL_MIN=1)
    sc, _ = family_scene(engine, 16, 3000, 80.0, (60, 238), 2100, spread=7)            # m = 1 with 2100 far-away hits: thousands of candidates
    ix = sc.index(world.mem)
    try:
        exp, got = check(ix, Frags(sc.sketches), 80.0, "pool retry", retry=True)
        assert len(exp.cand) > 20000
    finally:
        ix.close()


def case_hit_limit(world):
    """ANI_TEST_L1_HIT_LIMIT lowered: a fragment beyond it fails the call with ANI_ERR_LIMIT"""
    from fastani_amd.api import AniError
    engine = world.engine(ANI_TEST_L1_HIT_LIMIT=1000)
    sc, _ = family_scene(engine, 16, 3000, 80.0, (60,), 900, spread=7)
    ix = sc.index(world.mem)
    try:
        exp, got = check(ix, Frags(sc.sketches), 80.0, "hit limit, below")
        assert 900 < exp.hits.max() <= 1000
        c = sc.contig()
        sc.hits(238, [(c, 7 * i) for i in range(100)] + [(sc.contig(), 3)], [sc.pad_hash])      # 1001 hits: 101 of its own and the 900
        ix.close()
        ix = sc.index(world.mem)
        try:
            run_l1(ix, 0, Frags(sc.sketches))
        except AniError as err:
            assert err.code == ERR_LIMIT, err
        else:
            raise AssertionError("1001 seed hits passed a limit of 1000")
    finally:
        ix.close()


def case_max_s(world):
    """documented behaviour: the header's maxS sizes the minimumHits LUT (at least 512 entries); a sketch longer than the LUT gets m = 1"""
    sc = Scene(world.default, 16, 3000, 80.0, 41)
    assert sc.m(600) >= 2 and sc.m(238) == 2
    for s in (238, 512, 513, 600):
        c = sc.contig()
        sc.hits(s, [(c, 100)])                                         # one hit: a candidate only where m = 1
        c = sc.contig()
        sc.hits(s, [(c, 100 + i) for i in range(sc.m(s))])
    for max_s, lut in ((10, 512), (None, None)):
        ix = sc.index(world.mem)                                       # a sketch of its own: its LUT only grows
        try:
            exp, got = check(ix, Frags(sc.sketches, max_s=max_s), 80.0, "maxS %r" % max_s, lut_max_s=lut)
            assert [len(c) for c in exp.per] == ([0, 1, 0, 1, 1, 1, 1, 1] if lut else [0, 1] * 4)
        finally:
            ix.close()


CHUNK_RECORDS = 700


def case_chunks(world):
    """one record set in two or more index chunks (ANI_MAX_INDEX_MINIMIZERS): each chunk's candidates carry chunk-local seqIds and are
    the definition over that chunk's records alone"""
    engine = world.engine(ANI_MAX_INDEX_MINIMIZERS=CHUNK_RECORDS)
    sc = Scene(engine, 16, 3000, 80.0, 51)
    shared = sc.fresh(40)
    genome_contigs = []
    for g in range(4):
        cs = [sc.contig() for _ in range(3)]
        genome_contigs.append(3)
        at = 10
        for i in range(330):                                           # the same hashes in every genome, at other places
            sc.put(cs[i % 3], at, shared[(i * 7 + g) % 40] if i % 3 else sc.fresh(1)[0])
            at += int(sc.r.integers(1, 400))
    for f in range(30):
        sc.frag((60, 238, 20)[f % 3], [shared[(f + j * 3) % 40] for j in range(1 + f % 9)])
    ix = sc.index(world.mem, genome_contigs)
    try:
        ranges = ix.genome_ranges()
        assert len(ranges) >= 2, ranges
        total = 0
        for ch, (g0, g1) in enumerate(ranges):
            exp, got = check(ix, Frags(sc.sketches), 80.0, "chunk %d" % ch, chunk=ch, rec=ix.rset.chunk(g0, g1)[0])
            total += len(exp.cand)
            assert len(exp.cand) == 0 or exp.cand[:, 1].max() < ix.rset.gcs[g1] - ix.rset.gcs[g0]
        assert total > 0
    finally:
        ix.close()


def case_arguments(world):
    """what ani_l1_check refuses: null arguments, a chunk that does not exist, a fragment set of other parameters.  (A fragment set on
    another device needs two devices; a chunk that cannot be made resident needs a device without room for it.)"""
    engine = world.default
    sc = Scene(engine, 16, 3000, 80.0, 61)
    c = sc.contig()
    sc.hits(60, [(c, 5)])
    ix = sc.index(world.mem)
    lib = bind(engine.lib)
    frags = Frags(sc.sketches)
    try:
        wire = Buf(world.mem, frags.wire(ix.p))
        fset = FragmentSet.unpack(engine, wire.ptr, wire.init.nbytes, keepalive=wire)
        other = engine.params(16, 1000)
        wire2 = Buf(world.mem, frags.wire(other))
        fset2 = FragmentSet.unpack(engine, wire2.ptr, wire2.init.nbytes, keepalive=wire2)
        info = (ctypes.c_uint64 * 8)()
        out, words = ctypes.c_void_p(), ctypes.c_size_t()
        o, w = ctypes.byref(out), ctypes.byref(words)
        call = lib.ani_l1_check
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
        assert call(engine.h, ix.sk.h, 0, fset.h, info, o, w) == 0 and list(info)[:3] == [1, 1, frags.pool_size]
        engine.lib.ani_free(out)
        fset.close()
        fset2.close()
    finally:
        ix.close()
