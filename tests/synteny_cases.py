"""Cases for the synteny records (kernels/synteny.hpp: k_syn_list, k_syn_pairs, k_syn_compact; synteny_stage, syn_distribute and
ani_sketch_synteny_begin / _take / _end in engine_map.hip; --synteny of the command line), shared by the GPU tests (-m gpu, product
library) and the CPU-emulation tests (not gpu, tests/emu build): test_synteny.py.

The reference is a numpy restatement of rules 1 - 7 of include/ani_abi.h over ani_hit_t records: per pair the ranks of the querySeqIds
by argsort, the class of every adjacency, the maximal runs, their records.  In every engine case the hits and the synteny records are on
together and the synteny records must equal the restatement of the hits the SAME call returned (the hits themselves are held to their
own restatement and to the oracle by test_hits.py).  The hand-made lists carry their answers written out below.  Every comparison is on
whole record arrays; there is no tolerance."""
import ctypes

import numpy as np

import hits_cases as hc
import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import CI_DT, HIT_DT, SYNBLOCK_DT, SYNTENY_DT, FragmentSet, Sketch

bits = pc.bits
expect_error = pc.expect_error
PAIR_FIELDS = ("count", "forward", "reverse", "breaks", "contigBorders", "blocks", "reverseBlocks", "reverseHits", "largestBlock", "singletons")
TOP = 2 ** 31 - 1


def fix(identity):
    """llrint((double) identity * 2^20)"""
    return np.rint(np.asarray(identity, dtype=np.float32).astype(np.float64) * 1048576.0).astype(np.uint64)


# ---- rules 1 - 7 over hit records ----
def restate_pair(h):
    """one pair's hits in bin order -> (pair record, block records)"""
    n = len(h)
    q, c, p, F = h["querySeqId"].astype(np.int64), h["refSeqId"].astype(np.int64), h["refStartPos"], fix(h["identity"])
    assert len(np.unique(q)) == n, "the querySeqIds of a pair are distinct"
    r = np.argsort(np.argsort(q, kind="stable"), kind="stable")                  # rule 2
    contig = c[1:] != c[:-1]                                                      # rule 3
    d = r[1:] - r[:-1]
    forward, reverse = ~contig & (d == 1), ~contig & (d == -1)
    brk = ~contig & ~forward & ~reverse
    first = np.flatnonzero(np.concatenate([[True], contig | brk]))               # rule 4
    last = np.concatenate([first[1:], [n]]) - 1
    blocks = np.zeros(len(first), dtype=SYNBLOCK_DT)                              # rule 6
    blocks["refSeqId"], blocks["refStartFirst"], blocks["refStartLast"] = c[first], p[first], p[last]
    blocks["qSeqFirst"], blocks["qSeqLast"], blocks["hits"] = q[first], q[last], last - first + 1
    cum = np.concatenate([[0], np.cumsum(F.astype(object))])
    blocks["idSum"] = [int(cum[b + 1] - cum[a]) for a, b in zip(first, last)]
    rev = blocks["qSeqLast"] < blocks["qSeqFirst"]
    pair = np.zeros(1, dtype=SYNTENY_DT)                                          # rule 5
    pair["refGenomeId"], pair["qryGenomeId"], pair["count"] = h["refGenomeId"][0], h["qryGenomeId"][0], n
    pair["forward"], pair["reverse"], pair["breaks"], pair["contigBorders"] = forward.sum(), reverse.sum(), brk.sum(), contig.sum()
    pair["blocks"], pair["reverseBlocks"], pair["reverseHits"] = len(first), rev.sum(), blocks["hits"][rev].sum()
    pair["largestBlock"], pair["singletons"] = blocks["hits"].max(), (blocks["hits"] == 1).sum()
    x = pair[0]
    assert int(x["forward"]) + int(x["reverse"]) + int(x["breaks"]) + int(x["contigBorders"]) == n - 1
    assert int(x["blocks"]) == int(x["breaks"]) + int(x["contigBorders"]) + 1
    return pair, blocks


def restate(hits, keep=None):
    """the hit records of one call (pair after pair, rule 6 of the hits) -> (SYNTENY_DT[pairs], SYNBLOCK_DT[blocks]); keep(ref, qry, n):
    the pairs that pass a synteny gate other than the hits'"""
    pairs, blocks = [np.zeros(0, dtype=SYNTENY_DT)], [np.zeros(0, dtype=SYNBLOCK_DT)]
    if len(hits):
        key = (hits["qryGenomeId"].astype(np.int64) << 32) | hits["refGenomeId"].astype(np.int64)
        cut = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1], [True]]))
        assert len(np.unique(key[cut[:-1]])) == len(cut) - 1, "one run of records per pair"
        for a, b in zip(cut[:-1], cut[1:]):
            if keep is None or keep(int(hits["refGenomeId"][a]), int(hits["qryGenomeId"][a]), b - a):
                p, bl = restate_pair(hits[a:b])
                pairs.append(p)
                blocks.append(bl)
    return np.concatenate(pairs), np.concatenate(blocks)


def same(got, exp, what=""):
    """both lists, byte for byte"""
    for g, e, dt in ((got[0], exp[0], SYNTENY_DT), (got[1], exp[1], SYNBLOCK_DT)):
        assert g.dtype == dt and g.shape == e.shape, (what, dt.names[0], g.shape, e.shape)
        if np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(e).tobytes():
            bad = next(i for i in range(len(g)) if g[i].tobytes() != e[i].tobytes())
            raise AssertionError("%s: %s records differ, the first at %d of %d:\n%r\n%r" % (what, dt.names[0], bad, len(g), g[bad], e[bad]))
    return True


def keep_rows(rows, gate):
    """the pairs of `rows` that pass `gate`, as restate's keep"""
    ok = set((int(r["refGenomeId"]), int(r["qryGenomeId"])) for r in rows
             if int(r["countSeq"]) >= int(gate[1]) and int(bits(r["identity"])) >= pc.gate_bits(gate[0]))
    return lambda ref, qry, n: (ref, qry) in ok


def both(sk, call, gate=(0.0, 1), syn_gate=None):
    """one mapping call with the hits and the synteny records on -> rows, hits, (pairs, blocks)"""
    sk.hits_begin(*gate)
    sk.synteny_begin(*(gate if syn_gate is None else syn_gate))
    rows = call()
    hits, syn = sk.hits_take(), sk.synteny_take()
    sk.hits_end()
    sk.synteny_end()
    assert SYNTENY_DT.itemsize == 48 and SYNBLOCK_DT.itemsize == 32
    return rows, hits, syn


def check_call(sk, call, what, gate=(0.0, 1), exp_rows=None):
    rows, hits, syn = both(sk, call, gate)
    if exp_rows is not None:
        assert rc.same_rows(rows, exp_rows), what
    assert same(syn, restate(hits), what)
    assert int(syn[0]["count"].sum()) == len(hits) and int(syn[0]["blocks"].sum()) == len(syn[1]), what
    return rows, hits, syn


# ---- the hand-made lists: one query against the 129-bin genome, whose first contig has bins 0 .. 20 and whose second starts at bin 21 ----
# name -> (bins of the hits, their querySeqIds in bin order, the pair record's counters in PAIR_FIELDS order,
#          the blocks as (first bin, last bin, qSeqFirst, qSeqLast, hits))
HAND = {
    "n1": ([5], [7], (1, 0, 0, 0, 0, 1, 0, 0, 1, 1), [(5, 5, 7, 7, 1)]),
    "n2_forward": ([5, 6], [3, 4], (2, 1, 0, 0, 0, 1, 0, 0, 2, 0), [(5, 6, 3, 4, 2)]),
    "n2_reverse": ([5, 9], [10, 2], (2, 0, 1, 0, 0, 1, 1, 2, 2, 0), [(5, 9, 10, 2, 2)]),
    "identity": (list(range(10)), list(range(10)), (10, 9, 0, 0, 0, 1, 0, 0, 10, 0), [(0, 9, 0, 9, 10)]),
    "reversal": (list(range(10)), list(range(9, -1, -1)), (10, 0, 9, 0, 0, 1, 1, 10, 10, 0), [(0, 9, 9, 0, 10)]),
    "inversion": (list(range(10)), [0, 1, 2, 6, 5, 4, 3, 7, 8, 9], (10, 4, 3, 2, 0, 3, 1, 4, 4, 0), [(0, 2, 0, 2, 3), (3, 6, 6, 3, 4), (7, 9, 7, 9, 3)]),
    "translocation": (list(range(10)), [0, 1, 2, 7, 8, 9, 3, 4, 5, 6], (10, 7, 0, 2, 0, 3, 0, 0, 4, 0),
                      [(0, 2, 0, 2, 3), (3, 5, 7, 9, 3), (6, 9, 3, 6, 4)]),
    "alternating": (list(range(8)), [0, 4, 1, 5, 2, 6, 3, 7], (8, 0, 0, 7, 0, 8, 0, 0, 1, 8),
                    [(0, 0, 0, 0, 1), (1, 1, 4, 4, 1), (2, 2, 1, 1, 1), (3, 3, 5, 5, 1), (4, 4, 2, 2, 1), (5, 5, 6, 6, 1), (6, 6, 3, 3, 1), (7, 7, 7, 7, 1)]),
    "contig_border": ([18, 19, 20, 21, 22, 23], [0, 1, 2, 3, 4, 5], (6, 4, 0, 0, 1, 2, 0, 0, 3, 0), [(18, 20, 0, 2, 3), (21, 23, 3, 5, 3)]),
    "contig_border_reverse": ([19, 20, 21, 22], [3, 2, 1, 0], (4, 0, 2, 0, 1, 2, 2, 4, 2, 0), [(19, 20, 3, 2, 2), (21, 22, 1, 0, 2)]),
    "unmatched_between": ([0, 1, 2, 3, 4, 5], [10, 20, 35, 36, 100, 7], (6, 4, 0, 1, 0, 2, 0, 0, 5, 1), [(0, 4, 10, 100, 5), (5, 5, 7, 7, 1)]),
    "gaps_in_bins": ([2, 9, 30, 31, 40], [5, 6, 7, 8, 9], (5, 3, 0, 0, 1, 2, 0, 0, 3, 0), [(2, 9, 5, 6, 2), (30, 40, 7, 9, 3)]),
    "sparse_forward": ([0, 1, 2, 3, 4], [0, 70000, 2 ** 24 + 1, TOP - 1, TOP], (5, 4, 0, 0, 0, 1, 0, 0, 5, 0), [(0, 4, 0, TOP, 5)]),
    "sparse_reverse": ([0, 1, 2, 3, 4], [TOP, TOP - 1, 5, 1, 0], (5, 0, 4, 0, 0, 1, 1, 5, 5, 0), [(0, 4, TOP, 0, 5)]),
}


def hand_list(lay, name):
    """-> (mappings, the expected pair counters, the expected block records without ids) for the layout"""
    at, q, counters, blocks = HAND[name]
    gb = lay.genome_bins(rc.G129)
    assert [c for c, _ in gb[:43]] == [gb[0][0]] * 21 + [gb[21][0]] * 22 and gb[21][0] == gb[0][0] + 1     # the border the cases rely on
    contig = [gb[b][0] for b in at]
    pos = [gb[b][1] * lay.bin_w + 3 + (b % 5) for b in at]
    ident = (np.float32(80.0) + np.arange(len(at), dtype=np.float32) * np.float32(1.37)).astype(np.float32)
    maps = rc.mappings(lay, q, contig, pos, ident)
    F = [int(x) for x in fix(ident)]
    where = dict((b, i) for i, b in enumerate(at))
    exp = np.zeros(len(blocks), dtype=SYNBLOCK_DT)
    for k, (b0, b1, q0, q1, n) in enumerate(blocks):
        i0, i1 = where[b0], where[b1]
        exp[k] = (contig[i0], pos[i0], pos[i1], q0, q1, n, sum(F[i0:i1 + 1]))
    return maps, counters, exp


def hand_hits(lay, name, ref_id=rc.G129, qry_id=0):
    """the hit records the list must give (one mapping per fragment, one fragment per bin: every mapping is a hit)"""
    maps, _, _ = hand_list(lay, name)
    h = np.zeros(len(maps), dtype=HIT_DT)
    h["refGenomeId"], h["qryGenomeId"] = ref_id, qry_id
    h["refSeqId"], h["refStartPos"], h["querySeqId"], h["identity"] = maps["refSeqId"], maps["refStartPos"], maps["querySeqId"], maps["nucIdentity"]
    return h


def hand_expected(lay, name, qry_id=0):
    _, counters, blocks = hand_list(lay, name)
    pair = np.zeros(1, dtype=SYNTENY_DT)
    pair["refGenomeId"], pair["qryGenomeId"] = rc.G129, qry_id
    for f, v in zip(PAIR_FIELDS, counters):
        pair[f] = v
    return pair, blocks


def case_restatement(frag_len, name):
    """the restatement says what is written in HAND (CPU only, no engine)"""
    lay = rc.Layout(frag_len)
    assert same(restate(hand_hits(lay, name)), hand_expected(lay, name), name)


def case_hand(ref, name):
    lay, sk = ref.lay, ref.sk
    maps, _, _ = hand_list(lay, name)
    exp = hand_expected(lay, name, 3)
    for order in (rc.in_order, rc.shuffled):
        if len(maps) < 2 and order is rc.shuffled:
            continue
        rows, hits, syn = both(sk, lambda: sk.compute_cgi(order(maps), int(maps["querySeqId"].max()) + 1, 3))
        what = "%s, fragLen %d, %s" % (name, lay.frag_len, order.__name__)
        assert hc.same(hits, hand_hits(lay, name, qry_id=3), what)
        assert same(syn, exp, what)
    # all hand-made lists as queries of one table: the same records, pair after pair (querySeqIds above 2^24 do not fit a table of queries)
    names = [n for n in HAND if not n.startswith("sparse")]
    start, all_maps, exp_p, exp_b = [0], [], [], []
    for k, n in enumerate(names):
        m, _, _ = hand_list(lay, n)
        m = m.copy()
        m["querySeqId"] += start[-1]
        all_maps.append(m)
        p, b = hand_expected(lay, n, 11 + k)
        b = b.copy()
        b["qSeqFirst"] += start[-1]
        b["qSeqLast"] += start[-1]
        exp_p.append(p)
        exp_b.append(b)
        start.append(start[-1] + 128)
    if name == "n1":                                         # once per reference set
        rows, hits, syn = both(sk, lambda: rc.reduce_check(ref, np.concatenate(all_maps), start, 0, 11))
        assert same(syn, (np.concatenate(exp_p), np.concatenate(exp_b)), "the hand-made lists in one table") and same(syn, restate(hits))


# ---- the lists of reduce_cases.py ----
def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    maps, frags = hc.LISTS[name](lay)
    exp_rows = ref.expected(maps, frags, 4)
    for order in (rc.in_order, rc.shuffled):
        if len(maps) < 2 and order is rc.shuffled:
            continue
        _, hits, syn = check_call(sk, lambda: sk.compute_cgi(order(maps), frags, 4), "%s, fragLen %d, %s" % (name, lay.frag_len, order.__name__), exp_rows=exp_rows)
        assert len(syn[0]) == len(exp_rows) and np.array_equal(syn[0]["count"], exp_rows["countSeq"].astype(np.uint32))
    if name == "full":
        assert tuple(int(c) for c in syn[0]["count"]) == rc.BIN_TOTALS       # pairs of 1, 63, 64, 65, 128, 129 and 3 hits
        assert int(syn[0]["contigBorders"].sum()) > 0 and int(syn[0]["breaks"].sum()) > 0
    if name == "sparse_ids":
        assert int(maps["querySeqId"].max()) == TOP and int(hits["querySeqId"].max()) > 2 ** 30 and len(np.unique(np.diff(np.unique(hits["querySeqId"])))) > 3
    if name == "n0":
        assert len(syn[0]) == 0 and len(syn[1]) == 0


def case_many(ref, name, gated=False):
    lay, sk = ref.lay, ref.sk
    maps0, frags = hc.LISTS[name](lay)
    for n_query in ((3, 5) if gated else (1, 2, 5)):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (3, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                gate = pc.oracle_gate(ref, maps, start) if gated else (0.0, 1)
                exp_rows = rc.expected_many(ref, maps, start, 7)
                for order in (rc.in_order, rc.shuffled):
                    what = "%s, fragLen %d, %d queries %r, genomeBase %d, gate %r, %s" % (name, lay.frag_len, n_query, start, genome_base, gate, order.__name__)
                    _, hits, syn = check_call(sk, lambda: rc.reduce_check(ref, order(maps), start, genome_base, 7), what, gate, exp_rows)
                    kept = [r for r in exp_rows if int(r["countSeq"]) >= gate[1] and int(bits(r["identity"])) >= pc.gate_bits(gate[0])]
                    assert len(syn[0]) == len(kept) and (not gated or 0 < len(kept) < len(exp_rows)), what
                    assert [(int(r["refGenomeId"]), int(r["qryGenomeId"])) for r in syn[0]] == [(int(r["refGenomeId"]), int(r["qryGenomeId"])) for r in kept]


# ---- the size borders: a reference of its own with a genome of 300 bins ----
BIG_BINS = (300, 70)
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)


class BigLayout(rc.Layout):
    """two genomes of one contig each, of 300 and 70 bins"""

    def __init__(self, frag_len):
        self.frag_len, self.bin_w = frag_len, frag_len - 20
        self.genomes = [[(n - 1) * self.bin_w + 5] for n in BIG_BINS]
        self.contig_len = np.array([n for lens in self.genomes for n in lens], dtype=np.int64)
        self.contig_genome = np.array([g for g, lens in enumerate(self.genomes) for _ in lens], dtype=np.int64)
        self.contig_bins = self.contig_len // self.bin_w + 1
        self.genome_contigs = [np.flatnonzero(self.contig_genome == g) for g in range(len(self.genomes))]
        self.n_contigs = len(self.contig_len)
        assert self.bin_totals() == BIG_BINS


class BigRef:
    def __init__(self, engine, frag_len=1000):
        self.lay = BigLayout(frag_len)
        self.p = engine.params(rc.K, frag_len)
        self.engine = engine
        self.sk = Sketch(engine, self.p, self.lay.sequences())

    def close(self):
        self.sk.close()


def sizes_list(lay, collinear):
    """query k has SIZES[k] fragments, one mapping each into as many bins of the 300-bin genome (spread over it), and three into the
    70-bin genome; the fragments' order over the bins is the identity (collinear) or a random permutation"""
    r = rc.rng(51, lay.frag_len, int(collinear))
    q, c, pos, start = [], [], [], [0]
    for n in SIZES:
        binsA = np.sort(r.choice(BIG_BINS[0], n, replace=False))
        order = np.arange(n) if collinear else r.permutation(n)
        for i, b in enumerate(binsA):
            q.append(start[-1] + int(order[i]))
            c.append(0)
            pos.append(int(b) * lay.bin_w + int(r.integers(0, 5)))
        for i, b in enumerate(r.choice(BIG_BINS[1], 3, replace=False)):
            q.append(start[-1] + n + i)
            c.append(1)
            pos.append(int(b) * lay.bin_w + int(r.integers(0, 5)))
        start.append(start[-1] + n + 3 + int(r.integers(0, 5)))               # some fragments without mappings behind
    n = len(q)
    return rc.mappings(lay, q, c, pos, rc.full_mantissa(r, n)), start


def case_sizes(big, lds_cap=None):
    """pairs of 1, 2, 2^k - 1, 2^k, 2^k + 1 hits (k = 5, 6, 8) in one launch; with the LDS cap at 32 the pairs of 33 and more hits run
    in the device pool beside those of up to 32 in LDS"""
    lay, sk = big.lay, big.sk
    for collinear in (True, False):
        maps, start = sizes_list(lay, collinear)
        for order in (rc.in_order, rc.shuffled):
            what = "sizes, collinear %r, %s, cap %r" % (collinear, order.__name__, lds_cap)
            _, hits, syn = check_call(sk, lambda: rc.reduce_check(big, order(maps), start, 0, 0), what)
            pairs = syn[0]
            a = pairs[pairs["refGenomeId"] == 0]
            assert tuple(int(x) for x in a["count"]) == SIZES, what
            if lds_cap is not None:
                assert (a["count"] <= lds_cap).sum() >= 3 and (a["count"] > lds_cap).sum() >= 3 and lds_cap in a["count"] and lds_cap + 1 in a["count"]
            if collinear:
                assert np.array_equal(a["blocks"], np.ones(len(a), dtype=np.uint32)) and np.array_equal(a["forward"], a["count"] - 1)
            else:
                assert int(a["breaks"].sum()) > 300 and int(a["blocks"].max()) > 200
    # a full reversal of 257 hits: one reverse block across every slab and wave border
    n = 257
    binsA = np.arange(20, 20 + n)
    maps = rc.mappings(lay, np.arange(n)[::-1] * 3, [0] * n, binsA * lay.bin_w + 11, rc.full_mantissa(rc.rng(52), n))
    _, hits, syn = check_call(sk, lambda: sk.compute_cgi(maps, 3 * n, 0), "reversal of 257")
    assert [int(syn[0][f][0]) for f in PAIR_FIELDS] == [n, 0, n - 1, 0, 0, 1, 1, n, n, 0]
    b = syn[1][0]
    assert (int(b["qSeqFirst"]), int(b["qSeqLast"]), int(b["hits"])) == (3 * (n - 1), 0, n) and int(b["idSum"]) == int(fix(hits["identity"]).astype(object).sum())


def case_pieces(ref, piece):
    """ANI_TEST_SYNTENY_PIECE pairs per launch and copy: `random3` over 12 queries (more than 65 pairs) and `full` over one"""
    lay, sk = ref.lay, ref.sk
    maps, frags = hc.LISTS["random3"](lay)
    start = rc.split_queries(frags, 12, 12)
    _, hits, syn = check_call(sk, lambda: rc.reduce_check(ref, maps, start, 0, 3), "random3, twelve queries, piece %d" % piece)
    assert len(syn[0]) > 65
    maps, frags = hc.list_full(lay)
    _, hits, syn = check_call(sk, lambda: sk.compute_cgi(maps, frags, 0), "full, piece %d" % piece)
    assert len(syn[0]) == len(rc.BIN_TOTALS)


# ---- gate, life cycle, arguments ----
def case_gate_edges(ref):
    """the gate's own edges, and a synteny gate that differs from the hits' gate in the same call"""
    lay, sk = ref.lay, ref.sk
    maps, frags = rc.list_random(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    thr = np.sort(rows["identity"])[len(rows) // 2]
    above, below = np.nextafter(thr, np.float32(200.0)), np.nextafter(thr, np.float32(0.0))
    top = int(rows["countSeq"].max())
    mid = int(np.sort(rows["countSeq"])[len(rows) // 2])
    seen = set()
    for gate in ((-0.0, 1), (thr, 1), (below, 1), (above, 1), (0.0, mid), (0.0, mid + 1), (0.0, top), (100.0, 1), (0.0, top + 1)):
        # the hits open, the synteny records gated: the restatement of the open hits, restricted to the rows that pass
        got_rows, hits, syn = both(sk, lambda: rc.reduce_check(ref, maps, start, 0, 0), (0.0, 1), gate)
        assert rc.same_rows(got_rows, rows), gate
        assert len(hits) == int(rows["countSeq"].sum())
        assert same(syn, restate(hits, keep_rows(rows, gate)), repr(gate))
        seen.add(len(syn[0]))
        # the hits gated, the synteny records open
        _, hits2, syn2 = both(sk, lambda: rc.reduce_check(ref, maps, start, 0, 0), gate, (0.0, 1))
        assert same(syn2, restate(hits), "open beside %r" % (gate,)) and len(hits2) == int(syn[0]["count"].sum())
    assert 0 in seen and len(rows) in seen and len(seen) >= 4
    # everything gated out: NULL and 0 for both lists
    lib, chk = ref.engine.lib, ref.engine._chk
    sk.synteny_begin(100.0, 1)
    rc.reduce_check(ref, maps, start, 0, 0)
    pp, n, bp, m = ctypes.c_void_p(1), ctypes.c_size_t(5), ctypes.c_void_p(1), ctypes.c_size_t(5)
    chk(lib.ani_sketch_synteny_take(sk.h, ctypes.byref(pp), ctypes.byref(n), ctypes.byref(bp), ctypes.byref(m)))
    assert n.value == 0 and m.value == 0 and not pp.value and not bp.value
    sk.synteny_end()


def case_life_cycle(ref):
    lay, sk = ref.lay, ref.sk
    a_maps, a_frags = rc.list_random(lay)
    b_maps, b_frags = rc.list_ties(lay)
    a_maps = rc.in_order(a_maps)
    start = rc.split_queries(b_frags, 5, 5)
    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    _, _, exp_a = both(sk, lambda: sk.compute_cgi(a_maps, a_frags, 1))
    _, hits_b, exp_b = both(sk, lambda: rc.reduce_check(ref, b_maps, start, 0, 10))
    assert len(exp_a[0]) and len(exp_b[0]) and same(exp_b, restate(hits_b))
    cat = (np.concatenate([exp_a[0], exp_b[0]]), np.concatenate([exp_a[1], exp_b[1]]))
    # two calls, one take: call order; the second take is empty; rows are those of a run with the mode off
    sk.synteny_begin()
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.synteny_take(), cat, "two calls")
    p, b = sk.synteny_take()
    assert p.shape == (0,) and b.shape == (0,)
    # a take between two calls
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.synteny_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    assert same(first, exp_a) and same(sk.synteny_take(), exp_b)
    # begin twice: the second drops what is pending and takes the new gate
    sk.compute_cgi(a_maps, a_frags, 1)
    gate = pc.oracle_gate(ref, b_maps, start)
    sk.synteny_begin(*gate)
    rc.reduce_check(ref, b_maps, start, 0, 10)
    gated = restate(hits_b, keep_rows(off_b, gate))
    assert 0 < len(gated[0]) < len(exp_b[0])
    assert same(sk.synteny_take(), gated, "second begin")
    # the C call: the buffers are the caller's, released with ani_free
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    pp, n, bp, m = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_synteny_take(sk.h, ctypes.byref(pp), ctypes.byref(n), ctypes.byref(bp), ctypes.byref(m)))
    assert n.value == len(gated[0]) and m.value == len(gated[1]) and pp.value and bp.value
    raw = ctypes.string_at(pp.value, n.value * 48), ctypes.string_at(bp.value, m.value * 32)
    lib.ani_free(pp)
    lib.ani_free(bp)
    assert raw == (gated[0].tobytes(), gated[1].tobytes())
    # end: take and end are refused, mapping works and returns the same rows; nothing of before the end comes back
    rc.reduce_check(ref, b_maps, start, 0, 10)
    sk.synteny_end()
    expect_error(sk.synteny_take, "take after end")
    expect_error(sk.synteny_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.synteny_begin()
    assert len(sk.synteny_take()[0]) == 0
    sk.synteny_end()


def case_destroy_while_on(engine, frag_len=1000):
    ref = rc.Ref(engine, frag_len)
    maps, frags = rc.list_random(ref.lay)
    ref.sk.synteny_begin()
    ref.sk.compute_cgi(maps, frags, 0)
    ref.close()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    f32 = np.float32
    expect_error(sk.synteny_take, "take without begin")
    expect_error(sk.synteny_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.synteny_begin(v, 1), "minIdentity " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.synteny_begin(50.0, n), "minFragments %d" % n)
    expect_error(sk.synteny_take, "take after a refused begin")
    pp, n, bp, m = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
    refs = [ctypes.byref(pp), ctypes.byref(n), ctypes.byref(bp), ctypes.byref(m)]
    expect_error(lambda: chk(lib.ani_sketch_synteny_begin(None, 0.0, 1)), "begin(null)")
    expect_error(lambda: chk(lib.ani_sketch_synteny_take(None, *refs)), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_synteny_end(None)), "end(null)")
    # a refused begin leaves a running mode and its gate alone
    rows = ref.expected(maps, frags, 0)
    gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 1)
    _, hits, _ = both(sk, lambda: sk.compute_cgi(maps, frags, 0))
    exp = restate(hits, keep_rows(rows, gate))
    assert 0 < len(exp[0]) < len(rows)
    sk.synteny_begin(*gate)
    sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: sk.synteny_begin(101.0, 1), "minIdentity 101")
    expect_error(lambda: sk.synteny_begin(0.0, 0), "minFragments 0")
    for k in range(4):
        args = list(refs)
        args[k] = None
        expect_error(lambda: chk(lib.ani_sketch_synteny_take(sk.h, *args)), "take with null argument %d" % k)
    assert same(sk.synteny_take(), exp, "after refused begins")
    sk.compute_cgi(maps, frags, 0)
    assert same(sk.synteny_take(), exp, "the gate after refused begins")
    sk.synteny_begin(100.0, 2 ** 31 - 1)
    sk.synteny_begin(-0.0, 1)
    sk.synteny_end()


def case_together(ref):
    """--ci at the same gate: the blocks' hits add up to count, their idSum to ani_ci_t.sum, and the pair record's two identities hold;
    every mode on at once changes nothing, and the rows are those of a run with everything off"""
    import fragdist_cases as fc
    lay, sk = ref.lay, ref.sk
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 2)
    _, _, alone = both(sk, lambda: rc.reduce_check(ref, maps, start, 0, 0), gate)
    sk.ci_begin(50, 95.0, 3, *gate)
    sk.profile_begin(*gate)
    sk.fragdist_begin(fc.DEFAULT_EDGES, 0.0, 1)
    sk.paint_begin()
    got_rows, hits, syn = both(sk, lambda: rc.reduce_check(ref, maps, start, 0, 0), gate)
    ci = sk.ci_take()
    for end in (sk.ci_end, sk.profile_end, sk.fragdist_end, sk.paint_end):
        end()
    assert rc.same_rows(got_rows, rows) and same(syn, alone, "with every mode on") and same(syn, restate(hits))
    pairs, blocks = syn
    assert ci.dtype == CI_DT and 0 < len(ci) == len(pairs) < len(rows)
    off = np.concatenate([[0], np.cumsum(pairs["blocks"].astype(np.int64))])
    for i, p in enumerate(pairs):
        mine = blocks[off[i]:off[i + 1]]
        assert (int(ci[i]["refGenomeId"]), int(ci[i]["qryGenomeId"])) == (int(p["refGenomeId"]), int(p["qryGenomeId"]))
        assert int(mine["hits"].sum()) == int(p["count"]) == int(ci[i]["count"])
        assert int(mine["idSum"].astype(object).sum()) == int(ci[i]["sum"])
        assert int(p["forward"]) + int(p["reverse"]) + int(p["breaks"]) + int(p["contigBorders"]) == int(p["count"]) - 1
        assert int(p["blocks"]) == int(p["breaks"]) + int(p["contigBorders"]) + 1


# ---- end to end: the mapper's own mappings ----
def e2e_run(e2e, engine, config, alloc):
    """the inputs of hits_cases.EndToEnd: batch, kept sets, an id base and a merged set, the hits beside the synteny records"""
    genomes = e2e.genomes
    sk = Sketch(engine, e2e.p, genomes)
    if config in ("chunked", "streamed"):
        assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
    sets = [engine.fragment_set(e2e.p, genomes[:3]), engine.fragment_set(e2e.p, genomes[3:])]
    _, hits, syn = check_call(sk, lambda: sk.map_cgi_batch(genomes, 0), config + ", map_cgi_batch, gated", hc.E2E_GATE, e2e.rows)
    assert hc.same(hits, e2e.gated) and 0 < len(syn[0]) < len(e2e.rows)
    _, hits, syn = check_call(sk, lambda: sk.map_cgi_fragsets(sets, [0, 3]), config + ", map_cgi_fragsets", (0.0, 1), e2e.rows)
    assert hc.same(hits, e2e.open) and len(syn[0]) == len(e2e.rows)
    # related genomes in shuffled contigs: collinear runs, breaks and contig borders all occur
    assert int(syn[0]["forward"].sum()) > 50 and int(syn[0]["breaks"].sum()) > 0 and int(syn[0]["contigBorders"].sum()) > 0 and int(syn[0]["largestBlock"].max()) >= 5
    open_syn = syn
    # the hits open, the synteny records gated, in one call
    _, hits3, syn3 = both(sk, lambda: sk.map_cgi_fragsets(sets, [0, 3]), (0.0, 1), hc.E2E_GATE)
    assert hc.same(hits3, e2e.open) and same(syn3, restate(e2e.gated), config + ", gated beside open hits")
    # a take over two calls
    sk.synteny_begin()
    rows = np.concatenate([sk.map_cgi_fragset(sets[0], 0), sk.map_cgi_fragset(sets[1], 3)])
    assert rc.same_rows(rows, e2e.rows) and same(sk.synteny_take(), open_syn, config + ", map_cgi_fragset twice")
    sk.synteny_end()
    # a reference id base and query ids that do not start at 0
    sk.set_ref_id_base(500)
    moved = e2e.rows.copy()
    moved["refGenomeId"] += 500
    moved["qryGenomeId"] += 20
    _, hits, syn = check_call(sk, lambda: sk.map_cgi_fragsets(sets, [20, 23]), config + ", id base", hc.E2E_GATE, moved)
    assert int(syn[0]["refGenomeId"].min()) >= 500 and int(syn[0]["qryGenomeId"].min()) >= 20
    for s in sets:
        s.close()
    # a merged set with query ids of its own
    parts = [genomes[:2], genomes[2:3], genomes[3:6], genomes[6:]]
    bases = [40, -1, 50, 60]
    packed = [engine.fragment_set(e2e.p, g) for g in parts]
    pitch = (max(x.packed_bytes() for x in packed) + 255) // 256 * 256
    mbuf, mptr = alloc(pitch * len(packed) + 1024)
    mptr = (mptr + 255) // 256 * 256
    for i, x in enumerate(packed):
        x.pack_into(mptr + i * pitch, pitch)
        x.close()
    mv = FragmentSet.unpack_merged(engine, mptr, pitch, bases, keepalive=mbuf)
    _, hits, syn = check_call(sk, lambda: sk.map_cgi_fragset(mv, 7), config + ", merged set")
    assert sorted(set(int(x) for x in syn[0]["qryGenomeId"])) == [47, 48, 57, 58, 59, 67, 68]
    mv.close()
    sk.synteny_begin()
    sk.map_cgi_batch(genomes[:2], 0)
    sk.close()                                          # a sketch destroyed with the mode on and records pending releases them


# ---- the command line: --synteny ----
def synteny_lines(out_lines, paths, genomes, hits, p, frag_len, keep=None):
    """the .synteny and .synblocks files for the lines of the -o file, from the restatement of the hit records of one sketch over all
    references (query and reference ids = list positions)"""
    pairs, blocks = restate(hits, keep)
    first = np.concatenate([[0], np.cumsum(pairs["blocks"].astype(np.int64))])
    at = dict(((int(x["qryGenomeId"]), int(x["refGenomeId"])), i) for i, x in enumerate(pairs))
    index = dict((x, i) for i, x in enumerate(paths))
    first_contig = np.concatenate([[0], np.cumsum([len(g) for g in genomes])])
    syn, blk = [], []
    for line in out_lines:
        q, r = line.split("\t")[:2]
        i = at.get((index[q], index[r]))
        if i is None:
            continue
        x = pairs[i]
        den = int(x["count"]) - 1 - int(x["contigBorders"])
        syn.append("\t".join([q, r] + [str(int(x[f])) for f in PAIR_FIELDS] + ["%.4f" % ((int(x["forward"]) + int(x["reverse"])) / den) if den else "NA"]))
        q_off = hc.fragment_offsets([len(c) for c in genomes[index[q]]], p, frag_len)
        for b in blocks[first[i]:first[i + 1]]:
            c = int(b["refSeqId"]) - int(first_contig[index[r]])
            base = sum(len(s) for s in genomes[index[r]][:c])
            lo, hi = sorted((int(b["qSeqFirst"]), int(b["qSeqLast"])))
            d = "+" if b["qSeqLast"] > b["qSeqFirst"] else "-" if b["qSeqLast"] < b["qSeqFirst"] else "."
            mean = np.float32(float(int(b["idSum"])) / 1048576.0 / float(int(b["hits"])))
            blk.append("\t".join([q, r, d, str(q_off[lo]), str(q_off[hi] + frag_len - 1), str(base + int(b["refStartFirst"])),
                                  str(base + int(b["refStartLast"]) + frag_len - 1), str(int(b["hits"])), "%g" % float(mean)]))
    return syn, blk


def case_cli(binary, engine, tmp, frag_len):
    import os
    import subprocess
    family = hc.e2e_genomes()
    genomes = [family[i] for i in hc.CLI_GENOMES]
    paths = []
    for i, g in enumerate(genomes):
        paths.append(os.path.join(tmp, "g%d.fa" % i))
        rc.orc.write_fasta(paths[-1], g, names=["g%d_%d" % (i, j) for j in range(len(g))])
    al = os.path.join(tmp, "al.txt")
    open(al, "w").write("\n".join(paths) + "\n")
    common = ["--fragLen", str(frag_len), "-k", str(hc.E2E_K)]
    p = engine.params(hc.E2E_K, frag_len)

    def run(args, env=None, code=0):
        r = subprocess.run([binary] + common + args, capture_output=True, env=dict(os.environ, **(env or {})))
        assert r.returncode == code, (args, r.stderr.decode()[-2000:])
        return r

    def files(out):
        return dict((f[len(os.path.basename(out)):], open(os.path.join(tmp, f), "rb").read()) for f in os.listdir(tmp) if f.startswith(os.path.basename(out)))

    def lines(path):
        return open(path).read().splitlines()

    # every other file is byte-equal to the run without --synteny
    others = ["--matrix", "--hits", "--ci", "--paint"]
    plain, with_syn = os.path.join(tmp, "plain.out"), os.path.join(tmp, "syn.out")
    run(["--ql", al, "--rl", al, "-o", plain] + others)
    run(["--ql", al, "--rl", al, "-o", with_syn, "--synteny"] + others)
    want, got = files(plain), files(with_syn)
    assert sorted(want) == ["", ".ci", ".hits", ".matrix", ".paint", ".paintsum"] and sorted(got) == sorted(list(want) + [".synteny", ".synblocks"])
    for suffix in want:
        assert want[suffix] == got[suffix], suffix
    out_lines = lines(plain)
    assert len(out_lines) >= 9
    # the run's own .hits file is what the API's hit records say, and the two new files are the restatement of those records
    sk = Sketch(engine, p, genomes)
    sk.hits_begin()
    sk.map_cgi_batch(genomes, 0)
    hits = sk.hits_take()
    sk.close()
    assert lines(with_syn + ".hits") == hc.hit_lines(out_lines, paths, paths, genomes, genomes, hits, p, frag_len)
    exp_syn, exp_blk = synteny_lines(out_lines, paths, genomes, hits, p, frag_len)
    got_syn, got_blk = lines(with_syn + ".synteny"), lines(with_syn + ".synblocks")
    assert got_syn == exp_syn, next(((a, b) for a, b in zip(got_syn, exp_syn) if a != b), (len(got_syn), len(exp_syn)))
    assert got_blk == exp_blk, next(((a, b) for a, b in zip(got_blk, exp_blk) if a != b), (len(got_blk), len(exp_blk)))
    assert len(got_syn) == len(out_lines) and all(len(x.split("\t")) == 13 for x in got_syn) and all(len(x.split("\t")) == 9 for x in got_blk)
    dirs = set(x.split("\t")[2] for x in got_blk)
    assert len(dirs) >= 2, dirs
    # the same files from two device contexts over slices, a streamed chunked set, reference splits and a sketch file in blocks
    skf = os.path.join(tmp, "refs.anisk")
    variants = [(["--ql", al, "--rl", al], {"ANI_SLICE_BYTES": "40000"}, ["--devices", "0,0"]),
                (["--ql", al, "--rl", al], {"ANI_SLICE_BYTES": "40000", "ANI_MAX_INDEX_MINIMIZERS": "5000", "ANI_MAX_RESIDENT_CHUNKS": "1"}, []),
                (["--ql", al, "--rl", al, "--saveSketch", skf], {}, []),
                (["--ql", al, "--refSketch", skf], {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, [])]
    for k, (args, env, extra) in enumerate(variants):
        out = os.path.join(tmp, "var%d.out" % k)
        run(args + ["-o", out, "--synteny"] + extra, env)
        assert lines(out) == out_lines and lines(out + ".synteny") == got_syn and lines(out + ".synblocks") == got_blk, (k, args, env, extra)
    # -t splits (whole sets in memory, one device: -s)
    out = os.path.join(tmp, "split.out")
    run(["--ql", al, "--rl", al, "-o", out, "--synteny", "-t", "2", "-s"])
    assert lines(out) == out_lines and lines(out + ".synteny") == got_syn and lines(out + ".synblocks") == got_blk
    # one query against one reference with --visualize (ani_map_query and ani_compute_cgi per query): the lines of that pair
    out = os.path.join(tmp, "one.out")
    run(["-q", paths[1], "-r", paths[0], "-o", out, "--synteny", "--visualize"])
    mine = lambda xs: [x for x in xs if x.split("\t")[:2] == [paths[1], paths[0]]]
    assert lines(out + ".synteny") == mine(got_syn) and lines(out + ".synblocks") == mine(got_blk) and len(mine(got_blk)) >= 1
    # the gate
    ids = sorted(set(float(x.split("\t")[2]) for x in out_lines))
    gate = (float("%.4f" % ((ids[0] + ids[-1]) / 2)), 2)
    gated = os.path.join(tmp, "gated.out")
    run(["--ql", al, "--rl", al, "-o", gated, "--synteny", "--syntenyMinANI", str(gate[0]), "--syntenyMinFragments", str(gate[1])])
    kept = set(tuple(x.split("\t")[:2]) for x in out_lines if float(x.split("\t")[2]) > gate[0] and int(x.split("\t")[3]) >= gate[1])
    assert 0 < len(kept) < len(out_lines) and lines(gated) == out_lines
    assert lines(gated + ".synteny") == [x for x in got_syn if tuple(x.split("\t")[:2]) in kept]
    assert lines(gated + ".synblocks") == [x for x in got_blk if tuple(x.split("\t")[:2]) in kept]
    # the dependent options are refused by name without --synteny, and bad values before anything is mapped
    for opts, msg in ((["--syntenyMinANI", "90"], b"ERROR, --syntenyMinANI needs --synteny"),
                      (["--syntenyMinFragments", "5"], b"ERROR, --syntenyMinFragments needs --synteny"),
                      (["--synteny", "--syntenyMinANI", "-1"], b"--syntenyMinANI takes"), (["--synteny", "--syntenyMinANI", "100.5"], b"--syntenyMinANI takes"),
                      (["--synteny", "--syntenyMinANI", "nan"], b"--syntenyMinANI takes"), (["--synteny", "--syntenyMinFragments", "0"], b"--syntenyMinFragments takes")):
        r = run(["--ql", al, "--rl", al, "-o", os.path.join(tmp, "refused.out")] + opts, code=1)
        assert msg in r.stderr, (opts, r.stderr[-500:])
    assert not os.path.exists(os.path.join(tmp, "refused.out"))
