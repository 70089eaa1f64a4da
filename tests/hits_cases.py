"""Cases for the reciprocal best-hit records (kernels/hits.hpp: k_hits_owner, k_hits_claim, k_hits_flags, k_hits_list, k_hits_records;
hits_stage, collect_rows and ani_sketch_hits_begin / _take / _end in engine_map.hip; --hits of the command line), shared by the GPU tests
(-m gpu, product library) and the CPU-emulation tests (not gpu, tests/emu build): test_hits.py.

The reference is a numpy restatement of rules 1 - 6 of include/ani_abi.h over a mapping list: per (fragment, genome) the 1-way winner
under (identity bits, refSeqId, refStartPos); per cell the winners sorted by (identity bits, querySeqId), the last one is the hit; per
row that passes the gate the hits of the genome's cells in bin order.  The restatement is first held to the oracle: for every list the
per-pair counts and the float means in record order are the rows of orc.Sketch.compute_cgi, bit for bit (rule 5).  Every comparison is
on whole record arrays viewed as <u4; there is no tolerance.

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins) and the engines are those of reduce_cases.py."""
import ctypes

import numpy as np

import golden_cases as gc
import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import HIT_DT, FragmentSet, Sketch

ERR_ARG = rc.ERR_ARG
bits = pc.bits


# ---- rules 1 - 6 ----
def cell_hits(b, maps):
    """rules 1 and 2 for ONE query -> (cell, refSeqId, refStartPos, querySeqId, identity bits, contenders), one entry per non-empty cell
    in cell order; contenders = the number of fragments whose 1-way winner lies in the cell with the cell's bits"""
    if len(maps) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z, z
    frag = maps["querySeqId"].astype(np.int64)
    seq = maps["refSeqId"].astype(np.int64)
    pos = maps["refStartPos"].astype(np.int64)
    idb = bits(maps["nucIdentity"]).astype(np.int64)
    gen = b.contig_genome[seq]
    o = np.lexsort((pos, seq, idb, gen, frag))           # rule 1: the winner of a (fragment, genome) group is its last element
    last = np.ones(len(o), dtype=bool)
    last[:-1] = (frag[o][1:] != frag[o][:-1]) | (gen[o][1:] != gen[o][:-1])
    w = o[last]
    cell = b.contig_start[seq[w]] + pos[w] // b.bin_w
    o2 = np.lexsort((frag[w], idb[w], cell))             # rule 2: per cell the largest identity, then the largest querySeqId
    w, cell = w[o2], cell[o2]
    top = np.ones(len(w), dtype=bool)
    top[:-1] = cell[1:] != cell[:-1]
    first = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
    best = np.repeat(idb[w][top], np.diff(np.concatenate([first, [len(w)]])))
    contenders = np.add.reduceat((idb[w] == best).astype(np.int64), first)
    h = w[top]
    return cell[top], seq[h], pos[h], frag[h], idb[h], contenders


def records(b, rows, hits_of, gate=(0.0, 1), ref_base=0):
    """rules 3 - 6: the records of the pairs of `rows` (the rows a call returned, in its order) that pass the gate; hits_of(qryGenomeId)
    = cell_hits of that query; a row's genome is refGenomeId - ref_base.  Holds rule 5 against every row it uses."""
    min_bits, min_frag = pc.gate_bits(gate[0]), int(gate[1])
    out = []
    for row in rows:
        if int(row["countSeq"]) < min_frag or int(bits(row["identity"])) < min_bits:
            continue
        g = int(row["refGenomeId"]) - ref_base
        cell, seq, pos, frag, idb, _ = hits_of(int(row["qryGenomeId"]))
        m = (cell >= b.genome_start[g]) & (cell < b.genome_start[g + 1])
        n = int(m.sum())
        r = np.zeros(n, dtype=HIT_DT)
        r["refGenomeId"], r["qryGenomeId"] = row["refGenomeId"], row["qryGenomeId"]
        r["refSeqId"], r["refStartPos"], r["querySeqId"] = seq[m], pos[m], frag[m]
        r["identity"] = idb[m].astype(np.uint32).view(np.float32)
        assert n == int(row["countSeq"]), (n, row)                              # rule 5: the count ...
        s = np.float32(0.0)
        for x in r["identity"]:
            s = np.float32(s + x)
        assert np.float32(s / np.float32(n)).tobytes() == np.float32(row["identity"]).tobytes(), row      # ... and the mean, in record order
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, dtype=HIT_DT)


def same(got, exp, what=""):
    assert got.dtype == HIT_DT and HIT_DT.itemsize == 24, got.dtype
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    g, e = np.ascontiguousarray(got).view("<u4").reshape(-1, 6), np.ascontiguousarray(exp).view("<u4").reshape(-1, 6)
    if not np.array_equal(g, e):
        bad = np.flatnonzero((g != e).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, the first at %d:\n%r\n%r" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]]))
    return True


def hits_many(b, maps, start, first_id):
    out = {}
    for q in range(len(start) - 1):
        out[first_id + q] = cell_hits(b, maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])])
    return out


# ---- the lists added here ----
def list_cells(lay, which, seed=1, ident=None):
    """one fragment of its own per chosen cell: which(genome, number of bins) -> the bins of the genome (indices into genome_bins) to fill"""
    r = rc.rng(41, lay.frag_len, seed)
    c, pos = [], []
    for g in range(len(rc.BIN_TOTALS)):
        allb = lay.genome_bins(g)
        for i in which(g, len(allb)):
            x, j = allb[i]
            c.append(x)
            pos.append(lay.pos_in_bin(x, j, r))
    n = len(c)
    return rc.mappings(lay, r.permutation(n), c, pos, rc.full_mantissa(r, n) if ident is None else ident), n


def list_full(lay, seed=1):
    """every bin of every genome occupied: pairs of exactly 1, 63, 64, 65, 128, 129 and 3 records"""
    return list_cells(lay, lambda g, n: range(n), seed)


def list_slab_slots(lay, seed=1):
    """only bins 0, 63, 64, 127 and 128 of every genome that has them: prefix slots at the slab edges of the 64-wide walk"""
    return list_cells(lay, lambda g, n: [i for i in (0, 63, 64, 127, 128) if i < n], seed)


def list_past(lay, seed=1):
    """refStartPos equal to the contig length (the largest value accepted) on every contig, and a second fragment in each contig's bin 0"""
    r = rc.rng(42, lay.frag_len, seed)
    n = lay.n_contigs
    c = np.concatenate([np.arange(n), np.arange(n)])
    pos = np.concatenate([lay.contig_len, np.zeros(n, dtype=np.int64)])
    return rc.mappings(lay, r.permutation(2 * n), c, pos, rc.full_mantissa(r, 2 * n)), 2 * n


LISTS = {
    "full": list_full,
    "slab_slots": list_slab_slots,
    "random": rc.list_random,
    "random2": lambda lay: rc.list_random(lay, 2),
    "random3": lambda lay: rc.list_random(lay, 3, n=4000),
    "ties": rc.list_ties,
    "bin_edges": rc.list_bin_edges,
    "dense": rc.list_dense,
    "hot_bin": rc.list_hot_bin,
    "sparse_ids": rc.list_sparse_ids,
    "long_group_255": lambda lay: rc.list_long_group(lay, 255),
    "past": list_past,
    "n1": rc.list_single,
    "n0": rc.list_empty,
}
LISTS_ONE = tuple(LISTS)
LISTS_OTHER_CONFIGS = ("full", "random", "ties", "sparse_ids")
LISTS_MANY = ("full", "random", "ties", "bin_edges", "hot_bin")
LISTS_GATE = ("random", "ties", "bin_edges", "dense")
LISTS_RESTATE = tuple(n for n in LISTS if n != "n0")


# ---- the restatement against the oracle: CPU only, no engine ----
def case_restatement(frag_len, name):
    lay = rc.Layout(frag_len)
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    osk = pc.oracle_sketch(frag_len)
    ids = np.unique(maps["querySeqId"])
    starts = [[0, int(ids[-1]) + 1]]
    if len(ids) > 3:
        starts.append(sorted(set([0] + [int(x) for x in ids[rc.split_queries(len(ids), 3, 3)[1:-1]]] + [int(ids[-1]) + 1])))
    n_rec = 0
    for start in starts:
        for q in range(len(start) - 1):
            mine = maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])]
            rows = osk.compute_cgi(mine, max(frags, 1), q, frag_len)
            h = cell_hits(b, mine)
            rec = records(b, rows, lambda qid: h)                            # rule 5 is asserted inside, row by row
            assert len(rec) == int(rows["countSeq"].sum()) == len(h[0]), (name, frag_len, q)
            # the cells are those of the profile's restatement, and every record is one of the list's mappings
            cell = pc.cells(b, mine)
            assert np.array_equal(np.flatnonzero(cell), h[0]) and np.array_equal(cell[h[0]], h[4].astype(np.uint32))
            have = set(zip(mine["querySeqId"].tolist(), mine["refSeqId"].tolist(), mine["refStartPos"].tolist(), bits(mine["nucIdentity"]).tolist()))
            assert all((int(r["querySeqId"]), int(r["refSeqId"]), int(r["refStartPos"]), int(bits(r["identity"]))) in have for r in rec)
            n_rec += len(rec)
    assert n_rec >= 1
    if name == "full":
        rows = osk.compute_cgi(maps, frags, 0, frag_len)
        assert tuple(int(c) for c in rows["countSeq"]) == rc.BIN_TOTALS
    if name == "slab_slots":
        rows = osk.compute_cgi(maps, frags, 0, frag_len)
        assert tuple(int(c) for c in rows["countSeq"]) == (1, 1, 2, 3, 4, 5, 1)
    if name in ("ties", "hot_bin"):
        assert int(cell_hits(b, maps)[5].max()) >= (2 if name == "ties" else 1)


# ---- one query: ani_compute_cgi ----
def run_one(sk, maps, frags, qid, gate=(0.0, 1)):
    sk.hits_begin(*gate)
    rows = sk.compute_cgi(maps, frags, qid)
    got = sk.hits_take()
    sk.hits_end()
    return rows, got


def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    exp_rows = ref.expected(maps, frags, 4)
    h = cell_hits(b, maps)
    exp = records(b, exp_rows, lambda qid: h)
    assert len(exp) == len(h[0])
    for order in (rc.in_order, rc.shuffled):
        if len(maps) < 2 and order is rc.shuffled:
            continue
        rows, got = run_one(sk, order(maps), frags, 4)
        what = "%s, fragLen %d, %s" % (name, lay.frag_len, order.__name__)
        assert rc.same_rows(rows, exp_rows), what
        assert same(got, exp, what)
    if name == "full":
        assert [int((exp["refGenomeId"] == g).sum()) for g in range(len(rc.BIN_TOTALS))] == list(rc.BIN_TOTALS)
    if name == "sparse_ids":
        assert int(maps["querySeqId"].max()) == 2 ** 31 - 1 and len(np.unique(np.diff(np.unique(maps["querySeqId"])))) > 3
    if name == "past":
        assert (exp["refStartPos"] == lay.contig_len[exp["refSeqId"]]).sum() >= lay.n_contigs // 2
    if name == "n0":
        assert len(exp) == 0


def case_ties(ref):
    """rule 2 and rule 1 spelled out on hand-made mappings; the expected records are written down here, not taken from the restatement"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    r = rc.rng(43, lay.frag_len)
    bins129, bins128, bins63 = lay.genome_bins(rc.G129), lay.genome_bins(rc.G128), lay.genome_bins(rc.G63)
    f32 = np.float32
    v = f32(97.123456)
    below = np.nextafter(v, f32(0.0))
    assert int(bits(v)) - int(bits(below)) == 1
    rows_, want = [], {}                                  # (querySeqId, contig, pos, identity); cell -> (querySeqId, contig, pos, identity) or None

    def spot(cellspec, off=None):
        x, j = cellspec
        lo, hi = j * lay.bin_w, min((j + 1) * lay.bin_w - 1, int(lay.contig_len[x]))
        return x, (int(r.integers(lo, hi + 1)) if off is None else lo + off)

    # two fragments with bit-equal winners in one cell: the larger querySeqId
    A = bins129[70]
    for q in (5, 9):
        x, p = spot(A)
        rows_.append((q, x, p, v))
        if q == 9:
            want[A] = (9, x, p, v)
    # three, the largest in the middle of the list
    B = bins129[3]
    for q in (2, 17, 4):
        x, p = spot(B)
        rows_.append((q, x, p, v))
        if q == 17:
            want[B] = (17, x, p, v)
    # a larger querySeqId with the identity one mantissa bit lower loses
    C = bins129[100]
    x, p = spot(C)
    rows_.append((3, x, p, v))
    want[C] = (3, x, p, v)
    x, p = spot(C)
    rows_.append((20, x, p, below))
    # fragment 30: its 1-way winner (cell D, 90) loses D to fragment 31 (95); its other mapping (85) would have won the otherwise empty
    # cell E of the same genome: no record for 30, and E stays empty
    D, E = bins128[10], bins128[90]
    x, p = spot(D)
    rows_.append((30, x, p, f32(90.0)))
    x, p = spot(E)
    rows_.append((30, x, p, f32(85.0)))
    x, p = spot(D)
    rows_.append((31, x, p, f32(95.0)))
    want[D] = (31, x, p, f32(95.0))
    want[E] = None
    # the 1-way tie-break decides the bin: equal identities on two contigs -> the larger refSeqId; on one contig -> the larger position
    F, G = bins63[0], bins63[-1]
    assert F[0] < G[0]
    xf, pf = spot(F)
    xg, pg = spot(G)
    rows_ += [(40, xf, pf, v), (40, xg, pg, v)]
    want[F], want[G] = None, (40, xg, pg, v)
    H, I = bins129[5], bins129[6]
    assert H[0] == I[0]
    xh, ph = spot(H)
    xi, pi = spot(I)
    rows_ += [(41, xi, pi, v), (41, xh, ph, v)]
    want[H], want[I] = None, (41, xi, pi, v)
    q, c, pos, ident = zip(*rows_)
    maps = rc.mappings(lay, q, c, pos, ident)
    frags = 42
    exp_rows = ref.expected(maps, frags, 0)
    h = cell_hits(b, maps)
    exp = records(b, exp_rows, lambda qid: h)
    # the restatement says what is written above
    at = dict((int(cl), i) for i, cl in enumerate(h[0]))
    for (x, j), w in want.items():
        cl = int(b.contig_start[x]) + j
        if w is None:
            assert cl not in at, (x, j)
        else:
            i = at[cl]
            assert (int(h[3][i]), int(h[1][i]), int(h[2][i]), int(h[4][i])) == (w[0], w[1], w[2], int(bits(w[3]))), ((x, j), w)
    assert len(exp) == sum(1 for w in want.values() if w is not None) and 30 not in exp["querySeqId"] and 20 not in exp["querySeqId"]
    assert int(h[5].max()) == 3
    for order in (rc.in_order, rc.shuffled):
        rows, got = run_one(sk, order(maps), frags, 0)
        assert rc.same_rows(rows, exp_rows) and same(got, exp, "ties, " + order.__name__)


# ---- several queries in one table: ani_reduce_check ----
def case_many(ref, name, gated=False):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps0, frags = LISTS[name](lay)
    for n_query in ((3, 5) if gated else (1, 2, 5)):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (3, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                if first is None and n_query == 5:
                    # a query without mappings between two with
                    mid = (start[2], start[3])
                    maps = maps[(maps["querySeqId"] < mid[0]) | (maps["querySeqId"] >= mid[1])]
                gate = pc.oracle_gate(ref, maps, start) if gated else (0.0, 1)
                exp_rows = rc.expected_many(ref, maps, start, 7)
                hm = hits_many(b, maps, start, 7)
                exp = records(b, exp_rows, hm.__getitem__, gate)
                if gated:
                    kept = np.array([int(r["countSeq"]) >= gate[1] and int(bits(r["identity"])) >= pc.gate_bits(gate[0]) for r in exp_rows])
                    assert 0 < kept.sum() < len(kept) and 0 < len(exp) < int(exp_rows["countSeq"].sum())
                else:
                    assert len(exp) == int(exp_rows["countSeq"].sum())
                for order in (rc.in_order, rc.shuffled):
                    sk.hits_begin(*gate)
                    got_rows = rc.reduce_check(ref, order(maps), start, genome_base, 7)
                    got = sk.hits_take()
                    sk.hits_end()
                    what = "%s, fragLen %d, %d queries %r, genomeBase %d, gate %r, %s" % (name, lay.frag_len, n_query, start, genome_base, gate, order.__name__)
                    assert rc.same_rows(got_rows, exp_rows), what
                    assert same(got, exp, what)


def case_gate_edges(ref):
    """the gate's own edges on `random` over 5 queries: -0.0 is 0; a row on the identity threshold contributes and the next float above it
    shuts it out; countSeq = minFragments contributes and minFragments - 1 does not; a gated-out pair between two kept ones; everything
    gated out is n = 0 and a NULL pointer"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_random(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    hm = hits_many(b, maps, start, 0)
    thr = np.sort(rows["identity"])[len(rows) // 2]
    above = np.nextafter(thr, np.float32(200.0))
    below = np.nextafter(thr, np.float32(0.0))
    keep_at, keep_above = bits(rows["identity"]) >= bits(thr), bits(rows["identity"]) >= bits(above)
    assert keep_at.sum() > keep_above.sum() > 0
    assert any(keep_at[i - 1] and not keep_at[i] and keep_at[i + 1] for i in range(1, len(rows) - 1))       # a gated-out pair between two kept
    top = int(rows["countSeq"].max())
    mid = int(np.sort(rows["countSeq"])[len(rows) // 2])
    assert (rows["countSeq"] == mid - 1).any() or (rows["countSeq"] < mid).any()
    lib, chk = ref.engine.lib, ref.engine._chk
    for gate, n_pairs in (((-0.0, 1), len(rows)), ((thr, 1), int(keep_at.sum())), ((below, 1), int(keep_at.sum())), ((above, 1), int(keep_above.sum())),
                          ((0.0, mid), int((rows["countSeq"] >= mid).sum())), ((0.0, mid + 1), int((rows["countSeq"] >= mid + 1).sum())),
                          ((0.0, top), int((rows["countSeq"] == top).sum())), ((100.0, 1), 0), ((0.0, top + 1), 0)):
        exp = records(b, rows, hm.__getitem__, gate)
        assert len(np.unique(exp[["refGenomeId", "qryGenomeId"]])) == n_pairs, gate
        sk.hits_begin(*gate)
        got_rows = rc.reduce_check(ref, maps, start, 0, 0)
        if n_pairs == 0:
            rp, n = ctypes.c_void_p(1), ctypes.c_size_t(5)
            chk(lib.ani_sketch_hits_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
            assert n.value == 0 and not rp.value, gate
        else:
            assert same(sk.hits_take(), exp, repr(gate))
        sk.hits_end()
        assert rc.same_rows(got_rows, rows), gate


def case_pieces(ref, piece):
    """ANI_TEST_HITS_PIECE records per launch and copy: `full` (pairs of 1, 63, 64, 65, 128, 129 and 3 records) through one query and
    through five in one table, `hot_bin` and `random`"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = list_full(lay)
    exp_rows = ref.expected(maps, frags, 0)
    h = cell_hits(b, maps)
    exp = records(b, exp_rows, lambda qid: h)
    counts = [int((exp["refGenomeId"] == g).sum()) for g in range(len(rc.BIN_TOTALS))]
    assert counts == list(rc.BIN_TOTALS)
    # what the piece sizes are for: 64 ends a piece exactly at a pair border (1 + 63) and holds the 64-record pair alone; 65 holds the
    # 65-record pair exactly; every size has pairs larger than a piece
    assert max(counts) > piece and (piece != 64 or counts[0] + counts[1] == 64) and (piece not in (64, 65) or piece in counts)
    rows, got = run_one(sk, maps, frags, 0)
    assert rc.same_rows(rows, exp_rows) and same(got, exp, "full, piece %d" % piece)
    for name in ("full", "random", "hot_bin"):
        maps, frags = LISTS[name](lay)
        start = rc.split_queries(frags, 5, 5)
        exp_rows = rc.expected_many(ref, maps, start, 3)
        exp = records(b, exp_rows, hits_many(b, maps, start, 3).__getitem__)
        sk.hits_begin()
        got_rows = rc.reduce_check(ref, maps, start, 0, 3)
        got = sk.hits_take()
        sk.hits_end()
        assert rc.same_rows(got_rows, exp_rows) and same(got, exp, "%s, five queries, piece %d" % (name, piece))


# ---- life cycle and arguments ----
expect_error = pc.expect_error


def case_life_cycle(ref):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    a_maps, a_frags = rc.list_random(lay)
    b_maps, b_frags = rc.list_ties(lay)
    a_maps = rc.in_order(a_maps)
    a_rows = ref.expected(a_maps, a_frags, 1)
    start = rc.split_queries(b_frags, 5, 5)
    many_rows = rc.expected_many(ref, b_maps, start, 10)
    a_hits, b_hits = cell_hits(b, a_maps), hits_many(b, b_maps, start, 10)
    exp_a = records(b, a_rows, lambda qid: a_hits)
    exp_b = records(b, many_rows, b_hits.__getitem__)
    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    assert rc.same_rows(off_a, a_rows) and rc.same_rows(off_b, many_rows)
    # two calls, one take: call order; the second take is empty
    sk.hits_begin()
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.hits_take(), np.concatenate([exp_a, exp_b]), "two calls")
    assert sk.hits_take().shape == (0,)
    # a take between two calls
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.hits_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    assert same(first, exp_a) and same(sk.hits_take(), exp_b)
    # begin twice: the second drops what is pending and takes the new gate
    sk.compute_cgi(a_maps, a_frags, 1)
    gate = pc.oracle_gate(ref, b_maps, start)
    sk.hits_begin(*gate)
    rc.reduce_check(ref, b_maps, start, 0, 10)
    exp_gated = records(b, many_rows, b_hits.__getitem__, gate)
    assert 0 < len(exp_gated) < len(exp_b)
    assert same(sk.hits_take(), exp_gated, "second begin")
    # the C call: the buffer is the caller's, released with ani_free
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_hits_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
    assert n.value == len(exp_gated) and rp.value
    raw = ctypes.string_at(rp.value, n.value * HIT_DT.itemsize)
    lib.ani_free(rp)
    assert raw == exp_gated.tobytes()
    # end: take and end are refused, mapping works and returns the same rows; nothing of before the end comes back
    rc.reduce_check(ref, b_maps, start, 0, 10)
    sk.hits_end()
    expect_error(sk.hits_take, "take after end")
    expect_error(sk.hits_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.hits_begin()
    assert len(sk.hits_take()) == 0
    sk.hits_end()


def case_destroy_while_on(engine, frag_len=1000):
    """a sketch destroyed with the mode on and records pending releases them"""
    ref = rc.Ref(engine, frag_len)
    maps, frags = rc.list_random(ref.lay)
    ref.sk.hits_begin()
    ref.sk.compute_cgi(maps, frags, 0)
    ref.close()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    b = pc.bins_of(ref.lay)
    maps, frags = rc.list_random(ref.lay)
    f32 = np.float32
    expect_error(sk.hits_take, "take without begin")
    expect_error(sk.hits_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.hits_begin(v, 1), "minIdentity " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.hits_begin(50.0, n), "minFragments %d" % n)
    expect_error(sk.hits_take, "take after a refused begin")
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    expect_error(lambda: chk(lib.ani_sketch_hits_begin(None, 0.0, 1)), "begin(null)")
    expect_error(lambda: chk(lib.ani_sketch_hits_take(None, ctypes.byref(rp), ctypes.byref(n))), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_hits_end(None)), "end(null)")
    # a refused begin leaves a running mode and its gate alone
    rows = ref.expected(maps, frags, 0)
    gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 1)
    h = cell_hits(b, maps)
    exp = records(b, rows, lambda qid: h, gate)
    assert 0 < len(exp) < int(rows["countSeq"].sum())
    sk.hits_begin(*gate)
    sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: sk.hits_begin(101.0, 1), "minIdentity 101")
    expect_error(lambda: sk.hits_begin(0.0, 0), "minFragments 0")
    expect_error(lambda: chk(lib.ani_sketch_hits_take(sk.h, None, ctypes.byref(n))), "take(sk, null, n)")
    expect_error(lambda: chk(lib.ani_sketch_hits_take(sk.h, ctypes.byref(rp), None)), "take(sk, rec, null)")
    assert same(sk.hits_take(), exp, "after refused begins")
    sk.compute_cgi(maps, frags, 0)
    assert same(sk.hits_take(), exp, "the gate after refused begins")
    # the limits of the ranges are accepted
    sk.hits_begin(100.0, 2 ** 31 - 1)
    sk.hits_begin(-0.0, 1)
    sk.hits_end()


def case_together(ref):
    """the profile, the distributions and the hits on at once: each equals its result alone, rows equal a run with everything off"""
    import fragdist_cases as fc
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    p_gate, d_gate = pc.oracle_gate(ref, maps, start), (0.0, int(np.sort(rows["countSeq"])[len(rows) // 3]))
    h_gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 2)
    exp_h = records(b, rows, hits_many(b, maps, start, 0).__getitem__, h_gate)
    assert 0 < len(exp_h) < int(rows["countSeq"].sum())
    # each alone
    sk.hits_begin(*h_gate)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    alone_h = sk.hits_take()
    sk.hits_end()
    assert same(alone_h, exp_h, "alone")
    sk.fragdist_begin(fc.DEFAULT_EDGES, *d_gate)
    rc.reduce_check(ref, maps, start, 0, 0)
    alone_d = sk.fragdist_take()
    sk.fragdist_end()
    sk.profile_begin(*p_gate)
    rc.reduce_check(ref, maps, start, 0, 0)
    alone_p = pc.read_raw(sk)
    sk.profile_end()
    # all three
    sk.profile_begin(*p_gate)
    sk.fragdist_begin(fc.DEFAULT_EDGES, *d_gate)
    sk.hits_begin(*h_gate)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    assert pc.read_raw(sk) == alone_p and pc.same_profile(sk.profile_read(), pc.Profile(b, *p_gate).add_many(maps, start))
    assert fc.same(sk.fragdist_take(), alone_d, "with the hits on")
    assert same(sk.hits_take(), exp_h, "with the profile and the distributions on")
    sk.profile_end()
    sk.fragdist_end()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.hits_take(), exp_h, "after the others' end")
    sk.hits_end()


# ---- end to end: the mapper's own mappings ----
E2E_K = 16
E2E_FRAG_LENS = (3000, 1500)
E2E_GATE = (80.0, 4)


def e2e_genomes():
    return gc.evolved_family(5, 45000, 6, seg=(800, 5625)) + gc.evolved_family(6, 45000, 2, seg=(800, 4000))


class EndToEnd:
    """the eight genomes of e2e_genomes against themselves: each query's ani_map_query mappings, the restatement's hits over them and
    the rows, made once per half and fragment length by the default engine"""

    def __init__(self, engine, frag_len):
        self.frag_len = frag_len
        self.genomes = e2e_genomes()
        self.p = engine.params(E2E_K, frag_len)
        sk = Sketch(engine, self.p, self.genomes)
        self.n_minimizers = sk.stats()["minimizers"]
        contig_len = [len(c) for g in self.genomes for c in g]
        contig_genome = [g for g, cs in enumerate(self.genomes) for _ in cs]
        self.b = pc.Bins(contig_len, contig_genome, frag_len)
        self.hits, self.maps, rows = {}, {}, []
        sk.hits_begin()
        for qi, q in enumerate(self.genomes):
            maps, total = sk.map_query(q)
            assert len(sk.hits_take()) == 0                   # ani_map_query adds nothing
            self.maps[qi] = maps
            self.hits[qi] = cell_hits(self.b, maps)
            rows.append(sk.compute_cgi(maps, total, qi))
            assert same(sk.hits_take(), records(self.b, rows[-1], self.hits.__getitem__), "ani_compute_cgi of query %d" % qi)
        sk.close()                                            # destroyed with the mode on
        self.rows = np.concatenate(rows)
        self.open = records(self.b, self.rows, self.hits.__getitem__)
        self.gated = records(self.b, self.rows, self.hits.__getitem__, E2E_GATE)
        assert 0 < len(self.gated) < len(self.open) == int(self.rows["countSeq"].sum())
        # the cell competition is exercised: cells with more than one fragment whose 1-way winner lies in them
        self.contested = 0
        for qi, maps in self.maps.items():
            frag, seq, pos = maps["querySeqId"].astype(np.int64), maps["refSeqId"].astype(np.int64), maps["refStartPos"].astype(np.int64)
            gen = self.b.contig_genome[seq]
            o = np.lexsort((pos, seq, bits(maps["nucIdentity"]).astype(np.int64), gen, frag))
            last = np.ones(len(o), dtype=bool)
            last[:-1] = (frag[o][1:] != frag[o][:-1]) | (gen[o][1:] != gen[o][:-1])
            w = o[last]
            _, n = np.unique(self.b.contig_start[seq[w]] + pos[w] // self.b.bin_w, return_counts=True)
            self.contested += int((n > 1).sum())
        assert self.contested >= 20, self.contested

    def expect(self, rows, gate, ref_base=0, hits=None):
        return records(self.b, rows, (hits or self.hits).__getitem__, gate, ref_base)

    def run(self, engine, config, alloc):
        sk = Sketch(engine, self.p, self.genomes)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        sets = [engine.fragment_set(self.p, self.genomes[:3]), engine.fragment_set(self.p, self.genomes[3:])]
        sk.hits_begin(*E2E_GATE)
        assert rc.same_rows(sk.map_cgi_batch(self.genomes, 0), self.rows), config
        assert same(sk.hits_take(), self.gated, config + ", map_cgi_batch, gated")
        sk.hits_begin()
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [0, 3]), self.rows), config
        assert same(sk.hits_take(), self.open, config + ", map_cgi_fragsets")
        # one kept set per call, and a take over two calls
        rows = np.concatenate([sk.map_cgi_fragset(sets[0], 0), sk.map_cgi_fragset(sets[1], 3)])
        assert rc.same_rows(rows, self.rows) and same(sk.hits_take(), self.open, config + ", map_cgi_fragset twice")
        # a reference id base, and query ids that do not start at 0: the records carry the rows' ids, refSeqId stays the sketch's own
        sk.set_ref_id_base(500)
        moved = self.rows.copy()
        moved["refGenomeId"] += 500
        moved["qryGenomeId"] += 20
        hits = dict((q + 20, h) for q, h in self.hits.items())
        sk.hits_begin(*E2E_GATE)
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [20, 23]), moved), config
        assert same(sk.hits_take(), self.expect(moved, E2E_GATE, 500, hits), config + ", id base, map_cgi_fragsets")
        for s in sets:
            s.close()
        # a merged set with query ids of its own: slots of 2, 1 (left out), 3 and 2 genomes under ids 40.., -, 50.., 60..
        parts = [self.genomes[:2], self.genomes[2:3], self.genomes[3:6], self.genomes[6:]]
        bases = [40, -1, 50, 60]
        ids = {0: 40, 1: 41, 3: 50, 4: 51, 5: 52, 6: 60, 7: 61}
        packed = [engine.fragment_set(self.p, g) for g in parts]
        pitch = (max(x.packed_bytes() for x in packed) + 255) // 256 * 256
        mbuf, mptr = alloc(pitch * len(packed) + 1024)
        mptr = (mptr + 255) // 256 * 256
        for i, x in enumerate(packed):
            x.pack_into(mptr + i * pitch, pitch)
            x.close()
        mv = FragmentSet.unpack_merged(engine, mptr, pitch, bases, keepalive=mbuf)
        merged = moved[np.isin(moved["qryGenomeId"] - 20, list(ids))].copy()
        merged["qryGenomeId"] = [ids[int(q) - 20] + 7 for q in merged["qryGenomeId"]]
        hits = dict((ids[q] + 7, h) for q, h in self.hits.items() if q in ids)
        sk.hits_begin()
        assert rc.same_rows(sk.map_cgi_fragset(mv, 7), merged), config
        assert same(sk.hits_take(), self.expect(merged, (0.0, 1), 500, hits), config + ", merged set")
        mv.close()
        sk.close()                                          # a sketch destroyed with the mode on releases its list


# ---- the command line: --hits ----
CLI_GENOMES = (0, 1, 2, 6)                                  # three relatives (one in shuffled contigs, one with a second contig) and a stranger
CLI_VISUAL_PAIRS = ((1, 0), (2, 0), (2, 1))                 # (query, reference) of the one-to-one runs that also write .visual
MAX_TIED = 0.05


def fragment_offsets(lens, p, frag_len):
    """the first base of every fragment id of a query genome, over its contigs (computeMap.hpp:160-167)"""
    out, run = [], 0
    for n in lens:
        if n < p.windowSize or n < p.kmerSize or n < frag_len:
            out.append(run)
            run += n
            continue
        fc = n // frag_len
        for i in range(fc):
            out.append(run)
            run += frag_len if i != fc - 1 else frag_len + n % frag_len
    return out


def hit_lines(out_lines, q_paths, r_paths, genomes_q, genomes_r, rec, p, frag_len):
    """the .hits file for the lines of the -o file, from the Python API's records of one sketch over all references (query and reference
    ids = list positions)"""
    runs = {}
    for i, r in enumerate(rec):
        runs.setdefault((int(r["qryGenomeId"]), int(r["refGenomeId"])), []).append(i)
    qi, ri = dict((x, i) for i, x in enumerate(q_paths)), dict((x, i) for i, x in enumerate(r_paths))
    first_contig = np.concatenate([[0], np.cumsum([len(g) for g in genomes_r])])
    out = []
    for line in out_lines:
        q, r = line.split("\t")[:2]
        q_off = fragment_offsets([len(c) for c in genomes_q[qi[q]]], p, frag_len)
        for i in runs.get((qi[q], ri[r]), ()):
            x = rec[i]
            c = int(x["refSeqId"]) - int(first_contig[ri[r]])
            r0 = int(x["refStartPos"]) + sum(len(s) for s in genomes_r[ri[r]][:c])
            q0 = q_off[int(x["querySeqId"])]
            out.append("\t".join([q, r, "%g" % float(x["identity"]), "NA", "NA", "NA", str(q0), str(q0 + frag_len - 1), str(r0), str(r0 + frag_len - 1), "NA", "NA"]))
    return out


def case_cli(binary, engine, tmp, frag_len, full):
    """`full`: everything; else the one-to-one runs with --visualize only (a second fragment length)"""
    import os
    import subprocess
    family = e2e_genomes()
    genomes = [family[i] for i in CLI_GENOMES]
    assert any(len(g) > 2 for g in genomes) and any(len(g) == 2 for g in genomes)
    paths = []
    for i, g in enumerate(genomes):
        paths.append(os.path.join(tmp, "g%d.fa" % i))
        rc.orc.write_fasta(paths[-1], g, names=["g%d_%d" % (i, j) for j in range(len(g))])
    al = os.path.join(tmp, "al.txt")
    open(al, "w").write("\n".join(paths) + "\n")
    common = ["--fragLen", str(frag_len), "-k", str(E2E_K)]
    p = engine.params(E2E_K, frag_len)

    def run(args, env=None, code=0):
        r = subprocess.run([binary] + common + args, capture_output=True, env=dict(os.environ, **(env or {})))
        assert r.returncode == code, (args, r.stderr.decode()[-2000:])
        return r

    def files(out):
        return dict((f[len(os.path.basename(out)):], open(os.path.join(tmp, f), "rb").read()) for f in os.listdir(tmp) if f.startswith(os.path.basename(out)))

    def lines(path):
        return open(path).read().splitlines()

    # (b) one-to-one with --visualize: a .hits line whose cell has a unique maximum is the .visual line; the files have the same length
    cells_total = cells_tied = 0
    one = {}
    for q, r in CLI_VISUAL_PAIRS:
        out = os.path.join(tmp, "vis_%d_%d.out" % (q, r))
        plain = os.path.join(tmp, "visplain_%d_%d.out" % (q, r))
        run(["-q", paths[q], "-r", paths[r], "-o", plain, "--visualize"])
        run(["-q", paths[q], "-r", paths[r], "-o", out, "--visualize", "--hits"])
        got, want = files(out), files(plain)
        assert sorted(got) == ["", ".hits", ".visual"] and sorted(want) == ["", ".visual"]
        assert got[""] == want[""] and got[".visual"] == want[".visual"], (q, r)         # (a) for this mode
        hits, visual = lines(out + ".hits"), lines(out + ".visual")
        sk = Sketch(engine, p, [genomes[r]])
        maps, total = sk.map_query(genomes[q])
        sk.close()
        b = pc.Bins([len(c) for c in genomes[r]], [0] * len(genomes[r]), frag_len)
        contenders = cell_hits(b, maps)[5]
        assert len(hits) == len(visual) == len(contenders) > 5, (q, r, len(hits), len(visual), len(contenders))
        for i, n in enumerate(contenders):
            if n == 1:
                assert hits[i] == visual[i] and len(hits[i].split("\t")) == 12, (q, r, i, hits[i], visual[i])
        cells_total += len(contenders)
        cells_tied += int((contenders > 1).sum())
        one[q, r] = hits
    assert cells_tied <= MAX_TIED * cells_total, "%d of %d cells are tied: the comparison with .visual says too little" % (cells_tied, cells_total)
    if not full:
        return

    # (a) all-vs-all: with --hits every other file is byte-equal to the run without it
    others = ["--matrix", "--profile", "--fragDist"]
    plain, with_hits = os.path.join(tmp, "plain.out"), os.path.join(tmp, "hits.out")
    run(["--ql", al, "--rl", al, "-o", plain] + others)
    run(["--ql", al, "--rl", al, "-o", with_hits, "--hits"] + others)
    want, got = files(plain), files(with_hits)
    assert sorted(want) == ["", ".fragdist", ".matrix", ".profile"] and sorted(got) == sorted(list(want) + [".hits"])
    for suffix in want:
        assert want[suffix] == got[suffix], suffix
    out_lines = lines(plain)
    all_hits = lines(with_hits + ".hits")
    assert len(out_lines) >= 9
    # ... and the file is what the Python API's records say
    sk = Sketch(engine, p, genomes)
    sk.hits_begin()
    sk.map_cgi_batch(genomes, 0)
    rec = sk.hits_take()
    sk.close()
    exp = hit_lines(out_lines, paths, paths, genomes, genomes, rec, p, frag_len)
    assert all_hits == exp, "%d lines, expected %d; first difference %r" % (len(all_hits), len(exp), next(((a, b) for a, b in zip(all_hits, exp) if a != b), None))
    assert len(exp) == len(rec)                               # every pair with records has an -o line here

    # (c) ... and the one-to-one .hits files concatenated in the order of the -o file
    cat = []
    index = dict((x, i) for i, x in enumerate(paths))
    for line in out_lines:
        q, r = (index[x] for x in line.split("\t")[:2])
        if (q, r) not in one:
            out = os.path.join(tmp, "one_%d_%d.out" % (q, r))
            run(["-q", paths[q], "-r", paths[r], "-o", out, "--hits"])
            one[q, r] = lines(out + ".hits")
        assert len(one[q, r]) == int(line.split("\t")[3]), line
        cat += one[q, r]
    assert all_hits == cat

    # (d) the same file from two lists, from two device contexts over slices, from a streamed chunked set, and from a sketch file in blocks
    skf = os.path.join(tmp, "refs.anisk")
    variants = [(["--ql", al, "--rl", al], {"ANI_SLICE_BYTES": "40000"}, ["--devices", "0,0"]),
                (["--ql", al, "--rl", al], {"ANI_SLICE_BYTES": "40000", "ANI_MAX_INDEX_MINIMIZERS": "5000", "ANI_MAX_RESIDENT_CHUNKS": "1"}, []),
                (["--ql", al, "--rl", al], {"ANI_SLICE_BYTES": "40000", "ANI_CLI_QUERY_WAVE_BYTES": "1"}, ["--devices", "0,0"]),
                (["--ql", al, "--rl", al, "--saveSketch", skf], {}, []),
                (["--ql", al, "--refSketch", skf], {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, []),
                (["--ql", al, "--refSketch", skf], {"ANI_CLI_REF_BLOCK_BYTES": "30000", "ANI_SLICE_BYTES": "40000", "ANI_CLI_QUERY_WAVE_BYTES": "80000"}, ["--devices", "0,0"])]
    ql2 = os.path.join(tmp, "ql2.txt")
    open(ql2, "w").write("\n".join(paths[1:]) + "\n")
    for k, (args, env, extra) in enumerate(variants):
        out = os.path.join(tmp, "var%d.out" % k)
        r = run(args + ["-o", out, "--hits", "--matrix"] + extra, env)
        assert lines(out) == out_lines and lines(out + ".hits") == all_hits, (k, args, env, extra)
        if "ANI_CLI_REF_BLOCK_BYTES" in env:
            assert "blocks of genomes" in r.stderr.decode(), r.stderr.decode()[-1500:]
    # queries that are not the references: the lines of those queries
    out = os.path.join(tmp, "lists.out")
    run(["--ql", ql2, "--rl", al, "-o", out, "--hits"])
    assert lines(out) == [x for x in out_lines if x.split("\t")[0] != paths[0]]
    assert lines(out + ".hits") == [x for x in all_hits if x.split("\t")[0] != paths[0]]

    # pairs that --minFraction drops have no lines
    strict = os.path.join(tmp, "strict.out")
    run(["--ql", al, "--rl", al, "-o", strict, "--hits", "--minFraction", "0.9"])
    strict_lines = lines(strict)
    assert 0 < len(strict_lines) < len(out_lines)
    kept = set(tuple(x.split("\t")[:2]) for x in strict_lines)
    assert lines(strict + ".hits") == [x for x in all_hits if tuple(x.split("\t")[:2]) in kept]

    # the gate: a threshold between the lowest and the highest ANI of the -o lines, and two fragments
    ids = sorted(set(float(x.split("\t")[2]) for x in out_lines))
    assert ids[-1] - ids[0] > 0.01
    gate = (float("%.4f" % ((ids[0] + ids[-1]) / 2)), 2)
    gated = os.path.join(tmp, "gated.out")
    run(["--ql", al, "--rl", al, "-o", gated, "--hits", "--hitsMinANI", str(gate[0]), "--hitsMinFragments", str(gate[1])])
    assert lines(gated) == out_lines
    kept = set(tuple(x.split("\t")[:2]) for x in out_lines if float(x.split("\t")[2]) > gate[0] and int(x.split("\t")[3]) >= gate[1])
    assert 0 < len(kept) < len(out_lines)
    assert lines(gated + ".hits") == [x for x in all_hits if tuple(x.split("\t")[:2]) in kept]

    # (e) the dependent options are refused by name without --hits, and bad values before anything is mapped
    for opts, msg in ((["--hitsMinANI", "90"], b"ERROR, --hitsMinANI needs --hits"), (["--hitsMinFragments", "5"], b"ERROR, --hitsMinFragments needs --hits"),
                      (["--hits", "--hitsMinANI", "-1"], b"--hitsMinANI takes"), (["--hits", "--hitsMinANI", "100.5"], b"--hitsMinANI takes"),
                      (["--hits", "--hitsMinANI", "nan"], b"--hitsMinANI takes"), (["--hits", "--hitsMinFragments", "0"], b"--hitsMinFragments takes")):
        r = run(["--ql", al, "--rl", al, "-o", os.path.join(tmp, "refused.out")] + opts, code=1)
        assert msg in r.stderr, (opts, r.stderr[-500:])
    assert not os.path.exists(os.path.join(tmp, "refused.out"))
