"""Cases for the paint records (kernels/paint.hpp: k_paint_best, k_paint_second, k_paint_flags, k_paint_records; paint_stage, collect_rows,
ani_sketch_paint_begin / _take / _end and ani_paint_merge in engine_map.hip; --paint of the command line), shared by the GPU tests (-m gpu,
product library) and the CPU-emulation tests (not gpu, tests/emu build): test_paint.py.

The reference is a numpy restatement of rules 1 - 4 of include/ani_abi.h over a mapping list: per (fragment, genome) the 1-way winner
under (identity bits, refSeqId, refStartPos); per fragment the genomes ordered by (identity bits descending, genome id ascending); the
first with its winner, the second with its identity, the number of genomes.  Its 1-way winners are first held to the oracle: the cells
they fill are those of profile_cases.cells, and the rows those cells give are the rows of orc.Sketch.compute_cgi, bit for bit.  Every
comparison is on whole record arrays viewed as <u4; there is no tolerance.

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins) and the engines are those of reduce_cases.py."""
import ctypes

import numpy as np

import golden_cases as gc
import hits_cases as hc
import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import PAINT_DT, FragmentSet, Sketch, paint_merge

ERR_ARG = rc.ERR_ARG
bits = pc.bits
expect_error = pc.expect_error
LISTS = hc.LISTS
LISTS_ONE = hc.LISTS_ONE
LISTS_OTHER_CONFIGS = ("full", "random", "ties", "sparse_ids", "hot_bin")
LISTS_MANY = hc.LISTS_MANY
LISTS_RESTATE = hc.LISTS_RESTATE


# ---- rules 1 - 4 ----
def winners(contig_genome, maps):
    """rule 1 for ONE query -> (fragment, genome, refSeqId, refStartPos, identity bits) of every (fragment, genome) group's winner, int64
    arrays ordered by (fragment, genome)"""
    if len(maps) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z
    frag = maps["querySeqId"].astype(np.int64)
    seq = maps["refSeqId"].astype(np.int64)
    pos = maps["refStartPos"].astype(np.int64)
    idb = bits(maps["nucIdentity"]).astype(np.int64)
    gen = np.asarray(contig_genome, dtype=np.int64)[seq]
    keep = idb != 0
    frag, seq, pos, idb, gen = frag[keep], seq[keep], pos[keep], idb[keep], gen[keep]
    o = np.lexsort((pos, seq, idb, gen, frag))           # the winner of a (fragment, genome) group is its last element
    last = np.ones(len(o), dtype=bool)
    last[:-1] = (frag[o][1:] != frag[o][:-1]) | (gen[o][1:] != gen[o][:-1])
    w = o[last]
    return frag[w], gen[w], seq[w], pos[w], idb[w]


def records(contig_genome, maps, qid, ref_base=0):
    """rules 2 - 4 for ONE query: PAINT_DT, one record per fragment with a winner, querySeqId ascending"""
    frag, gen, seq, pos, idb = winners(contig_genome, maps)
    o = np.lexsort((gen, -idb, frag))                     # rule 2: per fragment, higher bits first, then the smaller genome
    frag, gen, seq, pos, idb = frag[o], gen[o], seq[o], pos[o], idb[o]
    first = np.flatnonzero(np.concatenate([[True], frag[1:] != frag[:-1]])) if len(frag) else np.zeros(0, dtype=np.int64)
    count = np.diff(np.concatenate([first, [len(frag)]]))
    r = np.zeros(len(first), dtype=PAINT_DT)
    r["qryGenomeId"], r["querySeqId"] = qid, frag[first]
    r["refGenomeId"], r["refSeqId"], r["refStartPos"] = gen[first] + ref_base, seq[first], pos[first]
    r["identity"] = idb[first].astype(np.uint32).view(np.float32)
    r["genomes"] = count
    two = count > 1
    r["secondGenomeId"] = -1
    r["secondGenomeId"][two] = gen[first[two] + 1] + ref_base
    r["secondIdentity"][two] = idb[first[two] + 1].astype(np.uint32).view(np.float32)
    return r


def records_many(contig_genome, maps, start, first_id, ref_base=0):
    out = [records(contig_genome, maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])], first_id + q, ref_base)
           for q in range(len(start) - 1)]
    return np.concatenate(out) if out else np.zeros(0, dtype=PAINT_DT)


def same(got, exp, what=""):
    assert got.dtype == PAINT_DT and PAINT_DT.itemsize == 40, got.dtype
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    g, e = np.ascontiguousarray(got).view("<u4").reshape(-1, 10), np.ascontiguousarray(exp).view("<u4").reshape(-1, 10)
    if not np.array_equal(g, e):
        bad = np.flatnonzero((g != e).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, the first at %d:\n%r\n%r" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]]))
    return True


# ---- the restatement against the oracle: CPU only, no engine ----
def case_restatement(frag_len, name):
    lay = rc.Layout(frag_len)
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    osk = pc.oracle_sketch(frag_len)
    frag, gen, seq, pos, idb = winners(lay.contig_genome, maps)
    # the winners fill the cells of the profile's restatement, and those cells give the oracle's rows
    cell = np.zeros(b.n_bins, dtype=np.uint32)
    np.maximum.at(cell, b.contig_start[seq] + pos // b.bin_w, idb.astype(np.uint32))
    assert np.array_equal(cell, pc.cells(b, maps))
    assert rc.same_rows(pc.rows_of(b, cell, frags, 3), osk.compute_cgi(maps, frags, 3, frag_len)), (name, frag_len)
    # every winner is a mapping of the list and no mapping of its group beats it
    have = set(zip(maps["querySeqId"].tolist(), maps["refSeqId"].tolist(), maps["refStartPos"].tolist(), bits(maps["nucIdentity"]).tolist()))
    assert all(x in have for x in zip(frag.tolist(), seq.tolist(), pos.tolist(), idb.tolist()))
    rec = records(lay.contig_genome, maps, 3)
    assert len(rec) == len(np.unique(maps["querySeqId"])) and int(rec["genomes"].sum()) == len(frag)
    # rule 2, record by record, in plain Python
    by_frag = {}
    for f, g, s, p, i in zip(frag.tolist(), gen.tolist(), seq.tolist(), pos.tolist(), idb.tolist()):
        by_frag.setdefault(f, []).append((-i, g, s, p))
    for r in rec:
        order = sorted(by_frag[int(r["querySeqId"])])
        assert (int(r["refGenomeId"]), int(r["refSeqId"]), int(r["refStartPos"]), int(bits(r["identity"]))) == (order[0][1], order[0][2], order[0][3], -order[0][0])
        assert int(r["genomes"]) == len(order)
        if len(order) > 1:
            assert (int(r["secondGenomeId"]), int(bits(r["secondIdentity"]))) == (order[1][1], -order[1][0])
        else:
            assert int(r["secondGenomeId"]) == -1 and int(bits(r["secondIdentity"])) == 0
    if name in ("random", "ties"):
        assert (rec["genomes"] > 1).any()
    if name == "random":
        assert (rec["genomes"] == 1).any()


# ---- one query: ani_compute_cgi ----
def run_one(sk, maps, frags, qid):
    sk.paint_begin()
    rows = sk.compute_cgi(maps, frags, qid)
    got = sk.paint_take()
    sk.paint_end()
    return rows, got


def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    maps, frags = LISTS[name](lay)
    exp_rows = ref.expected(maps, frags, 4)
    exp = records(lay.contig_genome, maps, 4)
    for order in (rc.in_order, rc.shuffled):
        if len(maps) < 2 and order is rc.shuffled:
            continue
        rows, got = run_one(sk, order(maps), frags, 4)
        what = "%s, fragLen %d, %s" % (name, lay.frag_len, order.__name__)
        assert rc.same_rows(rows, exp_rows), what
        assert same(got, exp, what)
    if name == "sparse_ids":
        assert int(exp["querySeqId"].max()) == 2 ** 31 - 1 and len(np.unique(np.diff(exp["querySeqId"].astype(np.int64)))) > 3
    if name == "n0":
        assert len(exp) == 0
    if name == "n1":
        assert len(exp) == 1 and int(exp["genomes"][0]) == 1 and int(exp["secondGenomeId"][0]) == -1


# ---- several queries in one table: ani_reduce_check ----
def case_many(ref, name):
    lay, sk = ref.lay, ref.sk
    maps0, frags = LISTS[name](lay)
    for n_query in (1, 2, 5):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                if first is None and n_query == 5:
                    mid = (start[2], start[3])               # a query without mappings between two with
                    maps = maps[(maps["querySeqId"] < mid[0]) | (maps["querySeqId"] >= mid[1])]
                exp_rows = rc.expected_many(ref, maps, start, 7)
                exp = records_many(lay.contig_genome, maps, start, 7)
                assert len(exp) == len(np.unique(maps["querySeqId"]))
                for order in (rc.in_order, rc.shuffled):
                    sk.paint_begin()
                    got_rows = rc.reduce_check(ref, order(maps), start, genome_base, 7)
                    got = sk.paint_take()
                    sk.paint_end()
                    what = "%s, fragLen %d, %d queries %r, genomeBase %d, %s" % (name, lay.frag_len, n_query, start, genome_base, order.__name__)
                    assert rc.same_rows(got_rows, exp_rows), what
                    assert same(got, exp, what)


# ---- hand-made lists; the expected records are written down here, the restatement is held to them too ----
def _spot(lay, g, i, off=0):
    """(contig, position) in bin i of genome g"""
    x, j = lay.genome_bins(g)[i]
    return x, min(j * lay.bin_w + off, int(lay.contig_len[x]))


def _expect(q, f, g, x, p, v, second=(-1, 0.0), genomes=1):
    r = np.zeros(1, dtype=PAINT_DT)
    r["qryGenomeId"], r["querySeqId"], r["refGenomeId"], r["refSeqId"], r["refStartPos"], r["identity"] = q, f, g, x, p, np.float32(v)
    r["secondGenomeId"], r["secondIdentity"], r["genomes"] = second[0], np.float32(second[1]), genomes
    return r


def case_hand_made(ref):
    """one candidate; one genome only; two genomes at equal bits (in one chunk where the set has one, in two where it is chunked: G63 is
    in the first chunk and G129 in a later one); three genomes where the second is not the best's runner-up inside its own genome; a
    (fragment, genome) run of 65 candidates; the first and the last fragment of the query"""
    lay, sk = ref.lay, ref.sk
    f32 = np.float32
    v = f32(97.123456)
    below = np.nextafter(v, f32(0.0))
    chunks = sk.chunks()
    if len(chunks) > 1:
        assert np.searchsorted(chunks, rc.G63, side="right") != np.searchsorted(chunks, rc.G129, side="right"), chunks
    rows_, want = [], []
    # fragment 0 (the first): one candidate
    x, p = _spot(lay, rc.G64, 5, 3)
    rows_.append((0, x, p, v))
    want.append(_expect(9, 0, rc.G64, x, p, v))
    # fragment 2: one genome, three candidates, the 1-way tie-break picks the larger position at equal bits
    x, p = _spot(lay, rc.G128, 7, 1)
    x2, p2 = _spot(lay, rc.G128, 7, 9)
    x3, p3 = _spot(lay, rc.G128, 2, 0)
    assert x == x2 and p2 > p
    rows_ += [(2, x, p, v), (2, x2, p2, v), (2, x3, p3, below)]
    want.append(_expect(9, 2, rc.G128, x2, p2, v))
    # fragment 5: G63 and G129 at equal bits: the smaller id first, the other the second at the same bits
    xa, pa = _spot(lay, rc.G129, 100, 4)
    xb, pb = _spot(lay, rc.G63, 10, 4)
    rows_ += [(5, xa, pa, v), (5, xb, pb, v)]
    want.append(_expect(9, 5, rc.G63, xb, pb, v, (rc.G129, v), 2))
    # fragment 6: the same with G65 one bit below: three genomes
    xc, pc_ = _spot(lay, rc.G65, 1, 0)
    rows_ += [(6, xa, pa, v), (6, xb, pb, v), (6, xc, pc_, below)]
    want.append(_expect(9, 6, rc.G63, xb, pb, v, (rc.G129, v), 3))
    # fragment 8: G129 has 99 and 98, G3 has 90, G64 has 95: the second is G64 at 95, not G129's own runner-up
    xd, pd = _spot(lay, rc.G129, 3, 0)
    xe, pe = _spot(lay, rc.G129, 90, 0)
    xf, pf = _spot(lay, rc.G3, 1, 2)
    xg, pg = _spot(lay, rc.G64, 40, 2)
    rows_ += [(8, xd, pd, f32(99.0)), (8, xe, pe, f32(98.0)), (8, xf, pf, f32(90.0)), (8, xg, pg, f32(95.0))]
    want.append(_expect(9, 8, rc.G129, xd, pd, f32(99.0), (rc.G64, f32(95.0)), 3))
    # fragment 11: 65 candidates to G129, the best in the middle, and one to G1
    bins = lay.genome_bins(rc.G129)
    for i in range(65):
        x, p = _spot(lay, rc.G129, i, i % 7)
        ident = f32(96.5) if i == 33 else f32(80.0 + 0.125 * i)
        rows_.append((11, x, p, ident))
        if i == 33:
            best = (x, p)
    assert len(bins) >= 65
    x1, p1 = _spot(lay, rc.G1, 0, 2)
    rows_.append((11, x1, p1, f32(96.0)))
    want.append(_expect(9, 11, rc.G129, best[0], best[1], f32(96.5), (rc.G1, f32(96.0)), 2))
    # fragment 19 (the last): one candidate in the last genome
    x, p = _spot(lay, rc.G3, 2, 0)
    rows_.append((19, x, p, below))
    want.append(_expect(9, 19, rc.G3, x, p, below))
    q, c, pos, ident = zip(*rows_)
    maps = rc.mappings(lay, q, c, pos, ident)
    want = np.concatenate(want)
    assert same(records(lay.contig_genome, maps, 9), want, "the restatement")
    for order in (rc.in_order, rc.shuffled):
        rows, got = run_one(sk, order(maps), 20, 9)
        assert rc.same_rows(rows, ref.expected(maps, 20, 9)) and same(got, want, "hand made, " + order.__name__)


def case_block_border(ref):
    """fragment 0 has 250 candidates, fragment 1 has 12 to one genome: its group crosses lane 256 of the candidate walk (where the
    set is one chunk); and fragments whose groups end and begin exactly at the border"""
    lay, sk = ref.lay, ref.sk
    r = rc.rng(51, lay.frag_len)
    n129, n128 = len(lay.genome_bins(rc.G129)), len(lay.genome_bins(rc.G128))
    q, c, pos = [], [], []
    for lead, tail in ((250, 12), (256, 3), (255, 1)):
        base = 10 * len(q)
        for i in range(lead):
            x, p = _spot(lay, rc.G129 if i % 2 else rc.G128, i % (n129 if i % 2 else n128), int(r.integers(0, 50)))
            q.append(base); c.append(x); pos.append(p)
        for i in range(tail):
            x, p = _spot(lay, rc.G65, i, int(r.integers(0, 50)))
            q.append(base + 1); c.append(x); pos.append(p)
        maps = rc.mappings(lay, q, c, pos, rc.full_mantissa(r, len(q)))
        exp = records(lay.contig_genome, maps, 0)
        rows, got = run_one(sk, maps, base + 2, 0)
        assert same(got, exp, "block border %d + %d" % (lead, tail))
        q, c, pos = [], [], []


def case_scan_border(ref, n):
    """n mapped fragments (255, 256, 257: the scan's block border) with gaps in the ids; they alternate between G63 and G129, so that a
    chunked set sees, chunk by chunk, mapped fragments with unmapped ones in between; every third also hits the other genome"""
    lay, sk = ref.lay, ref.sk
    r = rc.rng(52, lay.frag_len, n)
    q, c, pos = [], [], []
    ids = np.cumsum(r.integers(1, 4, n))
    for i, f in enumerate(ids.tolist()):
        for g in ((rc.G63, rc.G129) if i % 3 == 0 else ((rc.G63,) if i % 2 else (rc.G129,))):
            x, p = _spot(lay, g, int(r.integers(0, 60)), int(r.integers(0, 50)))
            q.append(f); c.append(x); pos.append(p)
    maps = rc.mappings(lay, q, c, pos, rc.full_mantissa(r, len(q)))
    exp = records(lay.contig_genome, maps, 2)
    assert len(exp) == n and (np.diff(exp["querySeqId"]) > 1).any()
    for order in (rc.in_order, rc.shuffled):
        rows, got = run_one(sk, order(maps), int(ids[-1]) + 1, 2)
        assert same(got, exp, "%d mapped fragments, %s" % (n, order.__name__))
    # the same through ani_reduce_check: three queries, the first and the last fragment of the table are mapped
    start = [0, int(ids[n // 3]), int(ids[2 * n // 3]), int(ids[-1]) + 1]
    maps0 = maps.copy()
    maps0["querySeqId"][maps0["querySeqId"] == ids[0]] = 0
    sk.paint_begin()
    rc.reduce_check(ref, maps0, start, 500, 2)
    got = sk.paint_take()
    sk.paint_end()
    exp = records_many(lay.contig_genome, maps0, start, 2)
    assert int(exp["querySeqId"][0]) == 0 and int(exp["querySeqId"][-1]) == start[-1] - 1
    assert same(got, exp, "%d mapped fragments, three queries" % n)


class ManyGenomes:
    """a reference set of 70 genomes of one 300-base contig each: one fragment hits 64 and 65 of them"""
    N = 70

    def __init__(self, engine):
        self.seqs = [[rc.rng_genome(7000 + g, 300)] for g in range(self.N)]
        self.p = engine.params(rc.K, 1000)
        self.engine = engine
        self.sk = Sketch(engine, self.p, self.seqs)
        self.contig_genome = np.arange(self.N)
        self.lay = rc.Layout(1000)            # for rc.mappings only (fragLen)

    def close(self):
        self.sk.close()


def case_many_genomes(world_ref):
    mg = world_ref
    r = rc.rng(53)
    f32 = np.float32
    for hit in (64, 65):
        q, c, pos, ident = [], [], [], []
        # fragment 3 hits `hit` genomes (in shuffled identity order), fragment 4 all 70 at two identities, fragment 6 one
        gs = r.permutation(mg.N)[:hit]
        vals = rc.full_mantissa(r, hit)
        for g, v in zip(sorted(gs.tolist()), vals):
            q.append(3); c.append(g); pos.append(int(r.integers(0, 300))); ident.append(v)
        for g in range(mg.N):
            q.append(4); c.append(g); pos.append(int(r.integers(0, 300))); ident.append(f32(90.0) if g % 5 else f32(91.0))
        q.append(6); c.append(mg.N - 1); pos.append(300); ident.append(f32(80.0))
        maps = rc.mappings(mg.lay, q, c, pos, ident)
        exp = records(mg.contig_genome, maps, 1)
        assert [int(x) for x in exp["genomes"]] == [hit, mg.N, 1]
        assert (int(exp["refGenomeId"][1]), int(exp["secondGenomeId"][1])) == (0, 5)
        for order in (rc.in_order, rc.shuffled):
            mg.sk.paint_begin()
            mg.sk.compute_cgi(order(maps), 7, 1)
            got = mg.sk.paint_take()
            mg.sk.paint_end()
            assert same(got, exp, "%d genomes, %s" % (hit, order.__name__))


# ---- pieces ----
def case_pieces(ref, piece):
    """ANI_TEST_PAINT_PIECE records per launch and copy"""
    lay, sk = ref.lay, ref.sk
    for name in ("random", "ties", "hot_bin"):
        maps, frags = LISTS[name](lay)
        exp = records(lay.contig_genome, maps, 0)
        assert len(exp) > 65
        rows, got = run_one(sk, maps, frags, 0)
        assert rc.same_rows(rows, ref.expected(maps, frags, 0)) and same(got, exp, "%s, piece %d" % (name, piece))
        start = rc.split_queries(frags, 5, 5)
        sk.paint_begin()
        rc.reduce_check(ref, maps, start, 0, 3)
        got = sk.paint_take()
        sk.paint_end()
        assert same(got, records_many(lay.contig_genome, maps, start, 3), "%s, five queries, piece %d" % (name, piece))
    # exactly `piece`, `piece` + 1 and 2 * `piece` records
    for n in sorted(set((piece, piece + 1, 2 * piece))):
        r = rc.rng(54, n)
        q = np.arange(n) * 2
        c = r.integers(0, lay.n_contigs, n)
        pos = (r.random(n) * (lay.contig_len[c] + 1)).astype(np.int64)
        maps = rc.mappings(lay, q, c, pos, rc.full_mantissa(r, n))
        rows, got = run_one(sk, maps, 2 * n, 0)
        assert same(got, records(lay.contig_genome, maps, 0), "%d records, piece %d" % (n, piece))


# ---- ani_paint_merge: the host function alone ----
def case_merge(lib):
    lay = rc.Layout(1000)
    n_gen = len(rc.BIN_TOTALS)
    empty = np.zeros(0, dtype=PAINT_DT)
    for name in ("random", "ties", "hot_bin", "full"):
        maps, frags = LISTS[name](lay)
        start = rc.split_queries(frags, 3, 3)
        whole = records_many(lay.contig_genome, maps, start, 5, ref_base=100)
        gen = lay.contig_genome[maps["refSeqId"]]
        one_sided = 0
        for cut in range(n_gen + 1):
            a = records_many(lay.contig_genome, maps[gen < cut], start, 5, ref_base=100)
            b = records_many(lay.contig_genome, maps[gen >= cut], start, 5, ref_base=100)
            assert same(paint_merge(a, b, lib), whole, "%s cut at %d" % (name, cut))
            assert same(paint_merge(b, a, lib), whole, "%s cut at %d, sides swapped" % (name, cut))
            ka = set(zip(a["qryGenomeId"].tolist(), a["querySeqId"].tolist()))
            kb = set(zip(b["qryGenomeId"].tolist(), b["querySeqId"].tolist()))
            one_sided += len(ka ^ kb)
        assert one_sided > 0 or name == "full"
        # three parts, folded
        a = records_many(lay.contig_genome, maps[gen < 2], start, 5, ref_base=100)
        b = records_many(lay.contig_genome, maps[(gen >= 2) & (gen < 5)], start, 5, ref_base=100)
        c = records_many(lay.contig_genome, maps[gen >= 5], start, 5, ref_base=100)
        assert same(paint_merge(paint_merge(a, b, lib), c, lib), whole) and same(paint_merge(a, paint_merge(c, b, lib), lib), whole)
        assert same(paint_merge(whole, empty, lib), whole) and same(paint_merge(empty, whole, lib), whole)
    assert paint_merge(empty, empty, lib).shape == (0,)
    # ties across the sides, written down: equal bits -> the smaller genome id is first, whichever side it is on
    v, w = np.float32(97.5), np.float32(96.25)
    a = np.concatenate([_expect(1, 4, 10, 3, 70, v, (12, w), 2), _expect(1, 9, 10, 3, 71, v), _expect(2, 0, 30, 8, 5, w, (31, w), 5)])
    b = np.concatenate([_expect(1, 4, 7, 1, 50, v, (8, v), 3), _expect(2, 0, 29, 6, 9, w), _expect(3, 1, 7, 1, 2, w)])
    want = np.concatenate([_expect(1, 4, 7, 1, 50, v, (8, v), 5), _expect(1, 9, 10, 3, 71, v), _expect(2, 0, 29, 6, 9, w, (30, w), 6), _expect(3, 1, 7, 1, 2, w)])
    assert same(paint_merge(a, b, lib), want, "ties") and same(paint_merge(b, a, lib), want, "ties, swapped")
    # a list out of order and null pointers are refused
    expect_error(lambda: paint_merge(a[::-1].copy(), b, lib), "first list out of order")
    expect_error(lambda: paint_merge(a, np.concatenate([b, b]), lib), "second list with a fragment twice")
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()

    def chk(rc_):
        if rc_ != 0:
            from fastani_amd.api import AniError
            raise AniError(rc_, "")
    expect_error(lambda: chk(lib.ani_paint_merge(None, 2, b.ctypes.data, len(b), ctypes.byref(rp), ctypes.byref(n))), "merge(null, 2, ...)")
    expect_error(lambda: chk(lib.ani_paint_merge(a.ctypes.data, len(a), None, 1, ctypes.byref(rp), ctypes.byref(n))), "merge(.., null, 1, ..)")
    expect_error(lambda: chk(lib.ani_paint_merge(a.ctypes.data, len(a), b.ctypes.data, len(b), None, ctypes.byref(n))), "merge(out = null)")
    expect_error(lambda: chk(lib.ani_paint_merge(a.ctypes.data, len(a), b.ctypes.data, len(b), ctypes.byref(rp), None)), "merge(n = null)")


# ---- life cycle and arguments ----
def case_life_cycle(ref):
    lay, sk = ref.lay, ref.sk
    a_maps, a_frags = rc.list_random(lay)
    b_maps, b_frags = rc.list_ties(lay)
    a_maps = rc.in_order(a_maps)
    start = rc.split_queries(b_frags, 5, 5)
    exp_a = records(lay.contig_genome, a_maps, 1)
    exp_b = records_many(lay.contig_genome, b_maps, start, 10)
    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    assert rc.same_rows(off_a, ref.expected(a_maps, a_frags, 1)) and rc.same_rows(off_b, rc.expected_many(ref, b_maps, start, 10))
    # two calls, one take: call order; the second take is empty
    sk.paint_begin()
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.paint_take(), np.concatenate([exp_a, exp_b]), "two calls")
    assert sk.paint_take().shape == (0,)
    # a take between two calls
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.paint_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    assert same(first, exp_a) and same(sk.paint_take(), exp_b)
    # a begin while on is refused and leaves the mode and what is pending alone
    sk.compute_cgi(a_maps, a_frags, 1)
    expect_error(sk.paint_begin, "begin while on")
    assert same(sk.paint_take(), exp_a, "after the refused begin")
    # the C call: the buffer is the caller's, released with ani_free; with nothing pending it is NULL
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_paint_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
    assert n.value == len(exp_b) and rp.value
    raw = ctypes.string_at(rp.value, n.value * PAINT_DT.itemsize)
    lib.ani_free(rp)
    assert raw == exp_b.tobytes()
    rp, n = ctypes.c_void_p(1), ctypes.c_size_t(5)
    chk(lib.ani_sketch_paint_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
    assert n.value == 0 and not rp.value
    # end: take and end are refused, mapping works and returns the same rows; nothing of before the end comes back
    rc.reduce_check(ref, b_maps, start, 0, 10)
    sk.paint_end()
    expect_error(sk.paint_take, "take after end")
    expect_error(sk.paint_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.paint_begin()
    assert len(sk.paint_take()) == 0
    sk.paint_end()


def case_destroy_while_on(engine, frag_len=1000):
    """a sketch destroyed with the mode on and records pending releases them"""
    ref = rc.Ref(engine, frag_len)
    maps, frags = rc.list_random(ref.lay)
    ref.sk.paint_begin()
    ref.sk.compute_cgi(maps, frags, 0)
    ref.close()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    expect_error(sk.paint_take, "take without begin")
    expect_error(sk.paint_end, "end without begin")
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    expect_error(lambda: chk(lib.ani_sketch_paint_begin(None)), "begin(null)")
    expect_error(lambda: chk(lib.ani_sketch_paint_take(None, ctypes.byref(rp), ctypes.byref(n))), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_paint_end(None)), "end(null)")
    sk.paint_begin()
    sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: chk(lib.ani_sketch_paint_take(sk.h, None, ctypes.byref(n))), "take(sk, null, n)")
    expect_error(lambda: chk(lib.ani_sketch_paint_take(sk.h, ctypes.byref(rp), None)), "take(sk, rec, null)")
    assert same(sk.paint_take(), records(ref.lay.contig_genome, maps, 0), "after refused takes")
    sk.paint_end()


def case_together(ref):
    """the profile, the distributions, the hits and the intervals beside the paint records: each equals its result with paint off, the
    rows equal a run with everything off, and the paint records equal theirs alone"""
    import fragdist_cases as fc
    lay, sk = ref.lay, ref.sk
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    exp = records_many(lay.contig_genome, maps, start, 0)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    p_gate = pc.oracle_gate(ref, maps, start)
    h_gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 2)

    def others(paint):
        sk.profile_begin(*p_gate)
        sk.fragdist_begin(fc.DEFAULT_EDGES, 0.0, 1)
        sk.hits_begin(*h_gate)
        sk.ci_begin(50, 95.0, 3)
        if paint:
            sk.paint_begin()
        got_rows = rc.reduce_check(ref, maps, start, 0, 0)
        out = (got_rows, pc.read_raw(sk), sk.fragdist_take(), sk.hits_take(), sk.ci_take(), sk.paint_take() if paint else None)
        sk.profile_end(), sk.fragdist_end(), sk.hits_end(), sk.ci_end()
        if paint:
            sk.paint_end()
        return out

    off, on = others(False), others(True)
    assert rc.same_rows(off[0], rows) and rc.same_rows(on[0], rows)
    assert off[1] == on[1] and fc.same(on[2], off[2], "with paint on") and hc.same(on[3], off[3], "with paint on")
    assert len(off[4]) > 0 and on[4].tobytes() == off[4].tobytes()
    assert len(off[3]) > 0 and same(on[5], exp, "beside the other four")
    sk.paint_begin()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.paint_take(), exp, "alone")
    sk.paint_end()


# ---- end to end: the mapper's own mappings ----
E2E_K = hc.E2E_K
E2E_FRAG_LENS = hc.E2E_FRAG_LENS


class EndToEnd:
    """the eight genomes of hits_cases.e2e_genomes as references; as queries those eight and a ninth, genome 0 with a stretch of
    unrelated sequence in it (fragments that map nowhere).  Per query the restatement over its ani_map_query mappings, made once per
    fragment length by the default engine."""

    def __init__(self, engine, frag_len):
        self.frag_len = frag_len
        self.refs = hc.e2e_genomes()
        anc = self.refs[0][0]
        chimera = np.concatenate([anc[:4 * frag_len], rc.rng_genome(991, 3 * frag_len), anc[4 * frag_len:9 * frag_len]])
        self.queries = self.refs + [[chimera]]
        self.p = engine.params(E2E_K, frag_len)
        sk = Sketch(engine, self.p, self.refs)
        self.n_minimizers = sk.stats()["minimizers"]
        self.contig_genome = np.array([g for g, cs in enumerate(self.refs) for _ in cs])
        self.maps, self.totals = {}, {}
        sk.paint_begin()
        for qi, q in enumerate(self.queries):
            self.maps[qi], self.totals[qi] = sk.map_query(q)
            assert len(sk.paint_take()) == 0                   # ani_map_query adds nothing
            sk.compute_cgi(self.maps[qi], self.totals[qi], qi)
            assert same(sk.paint_take(), self.expect([qi]), "ani_compute_cgi of query %d" % qi)
        sk.close()                                            # destroyed with the mode on
        last = self.expect([8])
        mapped = set(last["querySeqId"].tolist())
        assert 0 < len(mapped) < self.totals[8] and any(f not in mapped for f in range(4, 7)), (sorted(mapped), self.totals[8])
        everything = self.expect(range(9))
        assert (everything["genomes"] > 1).sum() > 20 and (everything["secondGenomeId"] >= 0).sum() > 20

    def expect(self, queries, ids=None, ref_base=0):
        out = [records(self.contig_genome, self.maps[q], ids[q] if ids else q, ref_base) for q in queries]
        return np.concatenate(out)

    def run(self, engine, config, alloc):
        sk = Sketch(engine, self.p, self.refs)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        plain = sk.map_cgi_batch(self.queries, 0)
        sets = [engine.fragment_set(self.p, self.queries[:3]), engine.fragment_set(self.p, self.queries[3:])]
        sk.paint_begin()
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 0), plain), config
        assert same(sk.paint_take(), self.expect(range(9)), config + ", map_cgi_batch")
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [0, 3]), plain), config
        assert same(sk.paint_take(), self.expect(range(9)), config + ", map_cgi_fragsets")
        # one kept set per call, and a take over two calls
        rows = np.concatenate([sk.map_cgi_fragset(sets[0], 0), sk.map_cgi_fragset(sets[1], 3)])
        assert rc.same_rows(rows, plain) and same(sk.paint_take(), self.expect(range(9)), config + ", map_cgi_fragset twice")
        # a reference id base, and query ids that do not start at 0
        sk.set_ref_id_base(500)
        sk.map_cgi_fragsets(sets, [20, 23])
        assert same(sk.paint_take(), self.expect(range(9), dict((q, q + 20) for q in range(9)), 500), config + ", id base, map_cgi_fragsets")
        for s in sets:
            s.close()
        # a merged set with query ids of its own: slots of 2, 1 (left out), 3 and 3 genomes under ids 40.., -, 50.., 60..
        parts = [self.queries[:2], self.queries[2:3], self.queries[3:6], self.queries[6:]]
        bases = [40, -1, 50, 60]
        ids = {0: 47, 1: 48, 3: 57, 4: 58, 5: 59, 6: 67, 7: 68, 8: 69}
        packed = [engine.fragment_set(self.p, g) for g in parts]
        pitch = (max(x.packed_bytes() for x in packed) + 255) // 256 * 256
        mbuf, mptr = alloc(pitch * len(packed) + 1024)
        mptr = (mptr + 255) // 256 * 256
        for i, x in enumerate(packed):
            x.pack_into(mptr + i * pitch, pitch)
            x.close()
        mv = FragmentSet.unpack_merged(engine, mptr, pitch, bases, keepalive=mbuf)
        sk.map_cgi_fragset(mv, 7)
        assert same(sk.paint_take(), self.expect(sorted(ids), ids, 500), config + ", merged set")
        mv.close()
        sk.close()                                          # a sketch destroyed with the mode on releases its list


# ---- the command line: --paint ----
def case_cli(binary, engine, tmp, frag_len):
    import os
    import subprocess
    e2e_refs = hc.e2e_genomes()
    anc = e2e_refs[0][0]
    chimera = [np.concatenate([anc[:4 * frag_len], rc.rng_genome(991, 3 * frag_len), anc[4 * frag_len:9 * frag_len]]), anc[:frag_len // 2]]
    genomes = [e2e_refs[1], e2e_refs[2], chimera]          # two relatives (several contigs) and the chimera with a contig shorter than a fragment
    refs = genomes[:2]                                      # the chimera is a query only: its unrelated stretch maps nowhere
    paths = []
    for i, g in enumerate(genomes):
        paths.append(os.path.join(tmp, "g%d.fa" % i))
        rc.orc.write_fasta(paths[-1], g, names=["g%d_%d" % (i, j) for j in range(len(g))])
    al = os.path.join(tmp, "al.txt")
    open(al, "w").write("\n".join(paths) + "\n")
    rl = os.path.join(tmp, "rl.txt")
    open(rl, "w").write("\n".join(paths[:len(refs)]) + "\n")
    common = ["--fragLen", str(frag_len), "-k", str(E2E_K)]
    p = engine.params(E2E_K, frag_len)

    def run(args, env=None):
        r = subprocess.run([binary] + common + args, capture_output=True, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, (args, r.stderr.decode()[-2000:])

    def files(out):
        return dict((f[len(os.path.basename(out)):], open(os.path.join(tmp, f), "rb").read()) for f in os.listdir(tmp) if f.startswith(os.path.basename(out)))

    others = ["--matrix", "--profile", "--fragDist", "--hits", "--ci"]
    plain, painted = os.path.join(tmp, "plain.out"), os.path.join(tmp, "paint.out")
    run(["--ql", al, "--rl", rl, "-o", plain] + others)
    run(["--ql", al, "--rl", rl, "-o", painted, "--paint"] + others)
    want, got = files(plain), files(painted)
    assert sorted(want) == ["", ".ci", ".fragdist", ".hits", ".matrix", ".profile"] and sorted(got) == sorted(list(want) + [".paint", ".paintsum"])
    for suffix in want:
        assert want[suffix] == got[suffix], suffix
    paint = got[".paint"].decode().splitlines()
    # ... the file is what the Python API's records say: one line per fragment, NA where there is no record
    sk = Sketch(engine, p, refs)
    sk.paint_begin()
    sk.map_cgi_batch(genomes, 0)
    rec = sk.paint_take()
    sk.close()
    first_contig = np.concatenate([[0], np.cumsum([len(g) for g in refs])])
    at = dict(((int(r["qryGenomeId"]), int(r["querySeqId"])), r) for r in rec)
    exp, counts, unmapped = [], [], []
    for qi, g in enumerate(genomes):
        lens = [len(c) for c in g]
        offs = hc.fragment_offsets(lens, p, frag_len)
        real, fid = [], 0
        for n in lens:                                      # a contig shorter than a fragment takes an id and has no fragment
            if n < p.windowSize or n < p.kmerSize or n < frag_len:
                fid += 1
                continue
            real += list(range(fid, fid + n // frag_len))
            fid += n // frag_len
        counts.append(len(real))
        unmapped.append(0)
        for f in real:
            head = [paths[qi], str(offs[f]), str(offs[f] + frag_len - 1)]
            if (qi, f) not in at:
                exp.append("\t".join(head + ["NA"] * 7))
                unmapped[-1] += 1
                continue
            r = at[qi, f]
            g_ref = int(r["refGenomeId"])
            r0 = int(r["refStartPos"]) + sum(len(s) for s in refs[g_ref][:int(r["refSeqId"]) - int(first_contig[g_ref])])
            sec = [paths[int(r["secondGenomeId"])], "%g" % float(r["secondIdentity"])] if int(r["secondGenomeId"]) >= 0 else ["NA", "NA"]
            exp.append("\t".join(head + [paths[g_ref], "%g" % float(r["identity"]), str(r0), str(r0 + frag_len - 1), str(int(r["genomes"]))] + sec))
    assert len(rec) > 20 and unmapped[2] >= 1 and sum(unmapped) < sum(counts)
    assert len(paint) == sum(counts)
    assert paint == exp, "first difference %r" % (next(((a, b) for a, b in zip(paint, exp) if a != b), None),)
    # .paintsum adds up to every query's fragment count; its lines follow from the .paint lines
    summ = [x.split("\t") for x in got[".paintsum"].decode().splitlines()]
    for qi in range(len(genomes)):
        mine = [x for x in summ if x[0] == paths[qi]]
        assert mine[-1][1] == "NA" and mine[-1][2] == str(unmapped[qi]) and mine[-1][4:] == ["NA", "NA"]
        assert sum(int(x[2]) for x in mine) == counts[qi]
        assert [int(x[2]) for x in mine[:-1]] == sorted((int(x[2]) for x in mine[:-1]), reverse=True)
        lines = [x.split("\t") for x in paint if x.split("\t")[0] == paths[qi] and x.split("\t")[3] != "NA"]
        for x in mine[:-1]:
            own = [y for y in lines if y[3] == x[1]]
            assert int(x[2]) == len(own) > 0 and int(x[5]) == sum(1 for y in own if y[7] == "1") and x[3] == "%.4f" % (len(own) / counts[qi])
            fix = sum(int(np.rint(np.float64(r["identity"]) * 1048576.0)) for r in rec if int(r["qryGenomeId"]) == qi and paths[int(r["refGenomeId"])] == x[1])
            assert x[4] == "%g" % np.float32(fix / 1048576.0 / len(own)), (x, fix)
        assert mine[-1][3] == "%.4f" % (unmapped[qi] / counts[qi])
    # the same files under many sub-batches, from a chunked streamed set, from two device contexts over slices, and from a sketch file in blocks
    skf = os.path.join(tmp, "refs.anisk")
    variants = [(["--ql", al, "--rl", rl], {"ANI_SUBBATCH_FRAGS": "20"}, []),
                (["--ql", al, "--rl", rl], {"ANI_SLICE_BYTES": "40000"}, ["--devices", "0,0"]),
                (["--ql", al, "--rl", rl], {"ANI_SLICE_BYTES": "40000", "ANI_MAX_INDEX_MINIMIZERS": "5000", "ANI_MAX_RESIDENT_CHUNKS": "1"}, []),
                (["--ql", al, "--rl", rl, "--saveSketch", skf], {}, []),
                (["--ql", al, "--refSketch", skf], {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, [])]
    for k, (args, env, extra) in enumerate(variants):
        out = os.path.join(tmp, "var%d.out" % k)
        run(args + ["-o", out, "--paint"] + extra, env)
        f = files(out)
        assert f[".paint"] == got[".paint"] and f[".paintsum"] == got[".paintsum"] and f[""] == got[""], (k, args, env, extra)
