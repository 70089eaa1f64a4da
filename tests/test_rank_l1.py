"""L1 on position ranks (kernels/l1.hpp): the seed hits are gathered, filtered and sorted as 32-bit ranks of the index's position order
and expanded to (seqId, wpos) only for the run rule.  The cases sit where rank space and position space differ — contig borders,
dense and sparse contigs, the rank tiles of the noise filter and their counters, every size of the 32-bit register sort, the highest
rank of a chunk — and every result is held to the sequential definition of l1_cases.py (computeMap.hpp:283-354), exactly.  Once on the
CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu), through ani_l1_check.

Every case runs under four engines: the wave kernel (default), class S and class M with the noise filter forced on
(ANI_TEST_L1_FILTER_MIN=0) and forced off, and the batched path (ANI_TEST_L1_LDS_MAX=0).  A case holds its hit pattern twice, in a
sketch of 238 hashes (m = 2; class S without the wave kernel) and one of 1100 (m > 2; class M without the wave kernel)."""
import numpy as np
import pytest

import index_cases as ic
import l1_cases as lc
from test_index_build import emu, gpu      # noqa: F401  (the two halves' World: engines and memory)

ENGINES = {
    "wave": dict(),
    "lds_filter": dict(ANI_TEST_L1_TINY=0, ANI_TEST_L1_FILTER_MIN=0),
    "lds_nofilter": dict(ANI_TEST_L1_TINY=0, ANI_TEST_L1_FILTER_MIN=100000),
    "batched": dict(ANI_TEST_L1_LDS_MAX=0),
}
S_SMALL, S_MID = 238, 1100                                                     # sketch sizes: class S / class M when the wave kernel is off
M32 = 0xffffffff


def engine_of(world, name, **more):
    env = dict(ENGINES[name], **more)
    return (world.engine(**env) if env else world.default), env


def tile_width(L):
    shift = 1
    while (1 << shift) < 2 * L:
        shift += 1
    return shift, 1 << shift


def filter_counters(p, shift, bits):
    """the two counter indices of rank p in the noise filter (l1_filter_tiles), to PLACE hits: the expectation does not depend on it"""
    return (((p >> shift) * 0x9E3779B1) & M32) >> (32 - bits), ((((p + (1 << (shift - 1))) >> shift) * 0x85EBCA77) & M32) >> (32 - bits)


def run(sc, world, name, env, what, genome_contigs=None, want=None):
    """the scene's fragments against its index (every chunk) = the definition; -> [Expect per chunk]"""
    ix = sc.index(world.mem, genome_contigs)
    try:
        out = []
        frags = lc.Frags(sc.sketches)
        for ch, (g0, g1) in enumerate(ix.genome_ranges()):
            exp, got = lc.check(ix, frags, sc.identity, "%s [%s] chunk %d" % (what, name, ch), chunk=ch, rec=ix.rset.chunk(g0, g1)[0], **lc.knobs(env))
            out.append(exp)
        routes = {k: sum(e.routes[k] for e in out) for k in ("tiny", "small", "mid", "big")}
        must = want or {"wave": ("tiny",), "lds_filter": ("small", "mid"), "lds_nofilter": ("small", "mid"), "batched": ("big",)}[name]
        assert all(routes[k] > 0 for k in must), (name, routes)
        return out
    finally:
        ix.close()


def fillers(sc, c, positions):
    for w, h in zip(positions, sc.fresh(len(positions))):
        sc.put(c, w, h)


# ---- (a) contig border ----
def border_scene(engine, genome_pad=0):
    """hits on the last m entries of one contig and the first m of the next: adjacent in rank, one candidate in each contig and none
    across; m - 1 hits at the end of a contig and one at the start of the next: no candidate.  genome_pad: a genome of that many records
    in front (another index chunk), so that the ranks are chunk-local and the chunk's first contig is not contig 0"""
    sc = lc.Scene(engine, 16, 3000, 80.0, 71)
    genome_contigs = []
    if genome_pad:
        fillers(sc, sc.contig(), [3 + 7 * i for i in range(genome_pad)])
        genome_contigs.append(1)
    marks = []
    for s in (S_SMALL, S_MID):
        m = sc.m(s)
        a, b = sc.contig(), sc.contig()
        fillers(sc, a, [5 * i for i in range(40)])
        fillers(sc, b, [1000 + 5 * i for i in range(40)])
        f2 = sc.hits(s, [(a, 500 + i) for i in range(m)] + [(b, 3 * i) for i in range(m)])
        a, b = sc.contig(), sc.contig()
        fillers(sc, a, [5 * i for i in range(40)])
        fillers(sc, b, [1000 + 5 * i for i in range(40)])
        f0 = sc.hits(s, [(a, 500 + i) for i in range(m - 1)] + [(b, 0)])
        marks.append((f2, f0))
    if genome_pad:
        genome_contigs.append(len(sc.contigs) - 1)
    return sc, marks, genome_contigs or None


def case_border(world, name):
    engine, env = engine_of(world, name)
    sc, marks, _ = border_scene(engine)
    (exp,) = run(sc, world, name, env, "contig border")
    for f2, f0 in marks:
        assert len(exp.per[f2]) == 2 and exp.per[f2][0][0] + 1 == exp.per[f2][1][0] and exp.per[f0] == [], (exp.per[f2], exp.per[f0])


def case_border_two_chunks(world, name):
    engine, env = engine_of(world, name, ANI_MAX_INDEX_MINIMIZERS=lc.CHUNK_RECORDS)
    sc, marks, genome_contigs = border_scene(engine, genome_pad=lc.CHUNK_RECORDS - 100)
    exps = run(sc, world, name, env, "contig border, second chunk", genome_contigs)
    assert len(exps) == 2 and len(exps[0].cand) == 0
    for f2, f0 in marks:                                                       # chunk-local seqIds: the padding genome's contig is not counted
        assert len(exps[1].per[f2]) == 2 and exps[1].per[f2][0][0] + 1 == exps[1].per[f2][1][0] and exps[1].per[f0] == []
    assert min(c[0] for f2, _ in marks for c in exps[1].per[f2]) == 0


# ---- (b) dense contig ----
def case_dense(world, name, L=1000):
    """every position a minimizer (rank = wpos): m hits that span exactly L - 1 form a candidate, at span L none — each once across a
    tile border of the filter's first tiling and once across one of its second"""
    engine, env = engine_of(world, name)
    sc = lc.Scene(engine, 16, L, 80.0, 72)
    shift, T = tile_width(L)
    c = sc.contig()
    marks = []
    for s, t0 in ((S_SMALL, 1), (S_MID, 4)):
        m = sc.m(s)
        for border, span in ((t0 * T, L - 1), (t0 * T + T // 2, L - 1), ((t0 + 1) * T, L), ((t0 + 1) * T + T // 2, L)):
            x0 = border - (m - 1)                                              # m - 1 hits in front of the border, the last one behind it
            assert filter_counters(x0, shift, 13) != filter_counters(x0 + span, shift, 13)
            marks.append((sc.hits(s, [(c, x0 + i) for i in range(m - 1)] + [(c, x0 + span)]), span == L - 1))
    taken = sc.contigs[c][1]
    fillers(sc, c, [w for w in range(6 * T + L + 10) if w not in taken])
    (exp,) = run(sc, world, name, env, "dense contig")
    assert sorted(sc.contigs[c][1]) == list(range(6 * T + L + 10))
    for f, ok in marks:
        assert len(exp.per[f]) == (1 if ok else 0), (f, ok, exp.per[f])


# ---- (c) sparse contig ----
def case_sparse(world, name):
    """entries L apart in wpos: m hits on consecutive entries are within m ranks of each other and span (m - 1) L positions — kept by
    the filter, rejected by the run rule, no candidate.  With the entries L - 1 apart there is one where m = 2 and none where m > 2."""
    engine, env = engine_of(world, name)
    sc = lc.Scene(engine, 16, 3000, 80.0, 73)
    L = sc.L
    marks = []
    for s in (S_SMALL, S_MID):
        m = sc.m(s)
        for step in (L, L - 1):
            c = sc.contig()
            fillers(sc, c, [7 + j * step for j in (0, 1, m + 2, m + 3)])
            marks.append((sc.hits(s, [(c, 7 + (2 + j) * step) for j in range(m)]), 1 if step == L - 1 and m == 2 else 0))
    (exp,) = run(sc, world, name, env, "sparse contig")
    for f, n in marks:
        assert len(exp.per[f]) == n and exp.hits[f] == exp.m_of[f], (f, n, exp.per[f])


# ---- (d) filter collisions ----
COLLIDE_L = 24                                                                  # tiles of 64 ranks: the smallest there is


def colliding_tiles(bits, shift):
    """three tiles of the second tiling whose counters are the same one, found from the function -> their first ranks + 5"""
    seen = {}
    for t in range(1, 1 << 16):
        p = (t << shift) - (1 << (shift - 1)) + 5
        seen.setdefault(filter_counters(p, shift, bits)[1], []).append(p)
        if len(seen[filter_counters(p, shift, bits)[1]]) == 3:
            return seen[filter_counters(p, shift, bits)[1]]
    raise AssertionError("no three colliding tiles")


def case_collisions(world, name):
    """three isolated hits whose tiles share a counter of the second tiling (13 bits in class S, 14 in class M; proved from the function
    first) and m hits in a row elsewhere: the one candidate of the m hits, as without the filter.  One dense contig, rank = wpos."""
    engine, env = engine_of(world, name)
    L = COLLIDE_L
    shift, T = tile_width(L)
    assert T == 64
    p = engine.params(16, L)
    p.percentageIdentity = 80.0
    plan = []
    for s, bits in ((S_SMALL, 13), (S_MID, 14)):
        three = colliding_tiles(bits, shift)
        assert len({filter_counters(x, shift, bits)[1] for x in three}) == 1 and len({(x + T // 2) >> shift for x in three}) == 3
        assert len({filter_counters(x, shift, bits)[0] for x in three}) == 3          # (the first tiling tells them apart)
        assert min(np.diff(three)) > 4 * L
        plan.append((s, three))
    n = max(max(three) for _, three in plan) + 70
    hashes = 2 * np.arange(n, dtype=np.uint32) + np.uint32(1)                  # the index: odd hashes; the fragments' own: even ones
    sketches, at = [], 0
    for j, (s, three) in enumerate(plan):
        m = lc.min_hits(s, 16, 80.0)
        ranks = list(three) + [1000 * (j + 1) + i for i in range(m)]
        mine = 2 * (np.arange(s, dtype=np.uint32) + np.uint32(at))
        at += s
        hashes[ranks] = mine[:len(ranks)]
        sketches.append(np.sort(mine))
    rset = ic.RecordSet([(n + 5, hashes, np.arange(n))])
    ix = ic.Index(engine, world.mem, p, rset)
    try:
        exp, got = lc.check(ix, lc.Frags(sketches), 80.0, "filter collisions [%s]" % name, **lc.knobs(env))
        assert [len(c) for c in exp.per] == [1, 1] and list(exp.hits) == [3 + lc.min_hits(s, 16, 80.0) for s, _ in plan]
    finally:
        ix.close()


# ---- (e) sort sizes ----
SORT_HITS = (511, 512, 513, 1023, 1025, 2031, 4080)


def case_sort_sizes(world, name):
    """fragments with 511 .. 4080 hits, none of them alone in its tiles (so the filter keeps them all): every size of block_sort<uint32_t>
    and its padding.  Seven hashes share the hits of a fragment, so the gathered ranks are seven interleaved ascending runs."""
    engine, env = engine_of(world, name)
    sc = lc.Scene(engine, 16, 3000, 80.0, 75)
    marks = []
    for s in (S_SMALL, S_MID):
        for H in SORT_HITS:
            c = sc.contig()
            hs = sc.fresh(7)
            at = int(sc.r.integers(0, 50))
            for i in range(H):
                sc.put(c, at, hs[(i * 3) % 7])
                at += int(sc.r.integers(1, 4))
            marks.append((sc.frag(s, hs), H))
    want = {"wave": ("small", "mid"), "batched": ("big",)}.get(name)
    (exp,) = run(sc, world, name, env, "sort sizes", want=want)
    for f, H in marks:
        assert exp.hits[f] == H and len(exp.per[f]) >= 1
    if name.startswith("lds"):
        assert exp.routes["small"] == len(SORT_HITS) - 1 and exp.routes["mid"] == len(SORT_HITS) + 1


# ---- (f) the highest rank ----
def case_highest_rank(world, name):
    """hits on the last entries of the chunk (p = n - 1 among them), and a chunk of one entry"""
    engine, env = engine_of(world, name)
    sc = lc.Scene(engine, 16, 3000, 80.0, 76)
    fillers(sc, sc.contig(), [11 * i for i in range(300)])
    last = sc.contig()
    fillers(sc, last, [4 * i for i in range(100)])
    base, marks = 500, []
    for s in (S_MID, S_SMALL):
        m = sc.m(s)
        marks.append(sc.hits(s, [(last, base + i) for i in range(m)]))
        base += m
    marks.append(sc.hits(60, [(last, base)]))                                  # m = 1: a single hit on p = n - 1
    assert sc.m(60) == 1
    (exp,) = run(sc, world, name, env, "highest rank", want={"lds_filter": ("small", "mid"), "lds_nofilter": ("small", "mid")}.get(name))
    assert sorted(sc.contigs[last][1])[-1] == base and [len(exp.per[f]) for f in marks] == [1, 1, 1]
    one = lc.Scene(engine, 16, 3000, 80.0, 77)
    f = one.hits(60, [(one.contig(), 17)])
    (exp,) = run(one, world, name, env, "one entry", want={"lds_filter": ("small",), "lds_nofilter": ("small",)}.get(name))
    assert exp.per[f] == [[0, 0, 17]]


CASES = {"border": case_border, "border_two_chunks": case_border_two_chunks, "dense": case_dense, "sparse": case_sparse,
         "sort_sizes": case_sort_sizes, "highest_rank": case_highest_rank}


# ---- the CPU-emulation build ----
@pytest.mark.parametrize("name", ENGINES)
@pytest.mark.parametrize("case", CASES)
def test_emu_case(emu, case, name):
    CASES[case](emu, name)


def test_emu_collisions(emu):
    """(the index of this case has 7 x 10^5 entries, which the emulation builds in ~12 s: once, under the engine whose kernels filter)"""
    case_collisions(emu, "lds_filter")


# ---- the product library on the device ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINES)
@pytest.mark.parametrize("case", CASES)
def test_gpu_case(gpu, case, name):
    CASES[case](gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINES)
def test_gpu_collisions(gpu, name):
    case_collisions(gpu, name)
