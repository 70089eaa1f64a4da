"""Cases for the per-pair fragment identity distributions (kernels/fragdist.hpp: k_fragdist_flags, k_fragdist_list, k_fragdist_records;
fragdist_stage, collect_rows and ani_sketch_fragdist_begin / _take / _end in engine_map.hip), shared by the GPU tests (-m gpu, product
library) and the CPU-emulation tests (not gpu, tests/emu build): test_fragdist.py.

The reference is a numpy restatement of rules 1 - 6 of include/ani_abi.h over the cells of profile_cases.py (themselves held to the
oracle's rows there): per row that passes the gate, the sorted bit patterns of the genome's non-empty cells, their count, the class
counts by searchsorted over the edges' bit patterns, the five order statistics by index and the integer sum.  The ids and the order
of the expected records are those of the rows the same call returned.  Every comparison is on bits; there is no tolerance.

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins) and the engines are those of
reduce_cases.py; the lists added here put 2, 3, 4, 5 and 8 cells on the 3- and 63-bin genomes (every rounding of the rank indices;
the 1-bin genome holds its one cell), values that differ in the lowest mantissa bits only (the last round of the radix select) and one
value in every cell (minimum = maximum: the select is skipped)."""
import ctypes

import numpy as np

import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import FRAGDIST_DT, Sketch

ERR_ARG = rc.ERR_ARG
FIX = pc.FIX
bits = pc.bits
DEFAULT_EDGES = tuple(float(e) for e in range(70, 100)) + (99.5, 99.9)          # the command line's: 32 edges, 33 classes


def edge_bits(edges):
    e = np.asarray(edges, dtype=np.float32).reshape(-1)
    return np.where(e == 0, np.float32(0.0), e).view(np.uint32)              # -0.0 counts as 0


# ---- rules 1 - 6 ----
def record_of(v, edges):
    """one pair: v = the bit patterns of its non-empty cells -> (count, min, q1, median, q3, max as bits, sum, hist)"""
    v = np.sort(np.asarray(v, dtype=np.uint32))
    c = len(v)
    assert c >= 1 and (v != 0).all()
    cls = np.searchsorted(edge_bits(edges), v, side="right")                # the number of edges <= x, on bit patterns
    # ... which for these values is the float comparison of rule 3
    assert np.array_equal(cls, np.searchsorted(np.asarray(edges, dtype=np.float32).reshape(-1), v.view(np.float32), side="right"))
    hist = np.bincount(cls, minlength=len(edges) + 1).astype(np.uint32)
    fix = np.rint(v.view(np.float32).astype(np.float64) * FIX).astype(np.uint64)
    stats = (v[0], v[(c - 1) // 4], v[(c - 1) // 2], v[3 * (c - 1) // 4], v[c - 1])
    return c, stats, int(fix.sum(dtype=np.uint64)), hist


def expected(b, rows, cell_of, edges, gate=(0.0, 1), ref_base=0):
    """the records of the pairs of `rows` (the rows a call returned, in its order) that pass the gate; cell_of(qryGenomeId) = that
    query's cells (profile_cases.cells); a row's genome is refGenomeId - ref_base"""
    min_bits, min_frag = pc.gate_bits(gate[0]), int(gate[1])
    rec, hist = [], []
    for row in rows:
        if int(row["countSeq"]) < min_frag or int(bits(row["identity"])) < min_bits:
            continue
        g = int(row["refGenomeId"]) - ref_base
        cell = cell_of(int(row["qryGenomeId"]))[int(b.genome_start[g]):int(b.genome_start[g + 1])]
        c, st, total, h = record_of(cell[cell != 0], edges)
        assert c == int(row["countSeq"]) and int(h.sum()) == c                # rule 1, and the classes cover every value
        r = np.zeros(1, dtype=FRAGDIST_DT)
        r["refGenomeId"], r["qryGenomeId"], r["count"], r["sum"] = row["refGenomeId"], row["qryGenomeId"], c, total
        for name, x in zip(("minIdentity", "q1", "median", "q3", "maxIdentity"), st):
            r[name] = np.uint32(x).view(np.float32)
        rec.append(r)
        hist.append(h)
    if not rec:
        return np.zeros(0, dtype=FRAGDIST_DT), np.zeros((0, len(edges) + 1), dtype=np.uint32)
    return np.concatenate(rec), np.stack(hist)


def same(got, exp, what=""):
    (gr, gh), (er, eh) = got, exp
    assert gr.dtype == FRAGDIST_DT and gh.dtype == np.uint32, (gr.dtype, gh.dtype)
    assert gr.shape == er.shape and gh.shape == eh.shape, (what, gr.shape, er.shape, gh.shape, eh.shape)
    if gr.tobytes() != er.tobytes():
        bad = [i for i in range(len(gr)) if gr[i].tobytes() != er[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, the first at %d:\n%r\n%r" % (what, len(bad), len(gr), bad[0], gr[bad[0]], er[bad[0]]))
    if not np.array_equal(gh, eh):
        bad = np.flatnonzero((gh != eh).any(axis=1))
        raise AssertionError("%s: %d histograms differ, the first at %d:\n%r\n%r" % (what, len(bad), bad[0], gh[bad[0]], eh[bad[0]]))
    assert np.array_equal(gh.sum(axis=1, dtype=np.uint64), gr["count"].astype(np.uint64)), what
    return True


# ---- the lists added here ----
def list_counts(lay, counts, seed=1):
    """counts: genome -> number of cells; every cell from one fragment of its own, in bins spread over the genome"""
    r = rc.rng(31, lay.frag_len, seed, *[x for kv in sorted(counts.items()) for x in kv])
    c, pos = [], []
    for g, n in sorted(counts.items()):
        allb = lay.genome_bins(g)
        assert n <= len(allb)
        for i in sorted(r.choice(len(allb), n, replace=False)):
            x, j = allb[i]
            c.append(x)
            pos.append(lay.pos_in_bin(x, j, r))
    n = len(c)
    return rc.mappings(lay, r.permutation(n), c, pos, rc.full_mantissa(r, n)), n


def list_low_bits(lay, seed=1):
    """list_dense (every bin of the 129- and the 65-bin genome) with identities that differ in the two lowest mantissa bits only: the
    first three rounds of the select see one digit, the last decides; and most values occur many times"""
    maps, n = rc.list_dense(lay, seed)
    r = rc.rng(32, lay.frag_len, seed)
    base = int(bits(np.float32(98.5)))
    maps["nucIdentity"] = (base + r.integers(0, 4, len(maps))).astype(np.uint32).view(np.float32)
    return maps, n


def list_byte_steps(lay, seed=1):
    """list_dense with identities that differ in one byte of the pattern each: every round of the select has to split them"""
    maps, n = rc.list_dense(lay, seed)
    r = rc.rng(33, lay.frag_len, seed)
    base = int(bits(np.float32(80.0)))
    step = np.array([1, 1 << 8, 1 << 16, 3 << 16], dtype=np.int64)
    maps["nucIdentity"] = (base + step[r.integers(0, 4, len(maps))] * r.integers(0, 8, len(maps))).astype(np.uint32).view(np.float32)
    assert maps["nucIdentity"].min() >= 80.0 and maps["nucIdentity"].max() <= 100.0
    return maps, n


def list_all_equal(lay, seed=1):
    """list_dense with one identity everywhere: 129 and 65 cells whose minimum is their maximum"""
    maps, n = rc.list_dense(lay, seed)
    maps["nucIdentity"] = np.float32(97.25)
    return maps, n


LISTS = dict((name, rc.LISTS[name][0]) for name in ("random", "ties", "bin_edges", "dense", "hot_bin", "last_bin_only", "n1", "n0"))
LISTS.update({
    "c2": lambda lay: list_counts(lay, {rc.G1: 1, rc.G3: 2, rc.G63: 2}),
    "c3": lambda lay: list_counts(lay, {rc.G3: 3, rc.G63: 3}),
    "c4": lambda lay: list_counts(lay, {rc.G3: 1, rc.G63: 4}),
    "c5": lambda lay: list_counts(lay, {rc.G1: 1, rc.G63: 5}),
    "c8": lambda lay: list_counts(lay, {rc.G3: 2, rc.G63: 8}),
    "low_bits": list_low_bits,
    "byte_steps": list_byte_steps,
    "all_equal": list_all_equal,
})
LISTS_ONE = tuple(LISTS)
LISTS_MANY = ("random", "ties", "bin_edges", "dense", "hot_bin", "low_bits")
LISTS_GATE = ("random", "ties", "bin_edges", "dense")
LISTS_RESTATE = ("random", "ties", "bin_edges", "dense", "hot_bin", "c2", "c3", "c4", "c5", "c8", "low_bits", "byte_steps", "all_equal")


def edge_sets(cell):
    """name -> edges, for the non-empty cells `cell` (bit patterns) of a list: none, one, 63, edges bit-equal to cells, all below every
    value, all above every value, and the command line's default"""
    v = np.unique(cell[cell != 0])
    out = {"none": (), "one": (90.0,), "max63": tuple(np.linspace(70.0, 100.0, 63).astype(np.float32)), "default": DEFAULT_EDGES,
           "below": (-0.0, 1.0, 2.5)}
    if len(v):
        assert float(v.view(np.float32).min()) > 2.5
        out["on_cell"] = tuple(v[np.unique(np.linspace(0, len(v) - 1, 5).astype(int))].view(np.float32))
        top = np.nextafter(v.view(np.float32).max(), np.float32(200.0))
        if top <= 100.0:
            out["above"] = (top,) if top == 100.0 else (top, np.float32(100.0))
    return out


def check_edge_sets(name, sets, exp_by_set, cell):
    """what the edge sets are for, from the expected records alone"""
    v = cell[cell != 0]
    if "on_cell" in sets:
        eb = edge_bits(sets["on_cell"])
        assert np.isin(eb, v).all()
        # a cell bit-equal to edge e sits in class e + 1 or above, never in class e
        assert (np.searchsorted(eb, eb, side="right") == np.arange(1, len(eb) + 1)).all()
    for key, col in (("below", -1), ("above", 0)):
        if key in exp_by_set and len(exp_by_set[key][0]):
            rec, hist = exp_by_set[key]
            assert np.array_equal(hist[:, col], rec["count"]), (name, key)


# ---- the restatement against the oracle: CPU only, no engine ----
def case_restatement(frag_len, name):
    lay = rc.Layout(frag_len)
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    osk = pc.oracle_sketch(frag_len)
    start = rc.split_queries(frags, 3, 3) if frags > 3 else [0, frags]
    n_rec = 0
    for q in range(len(start) - 1):
        mine = maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])]
        rows = osk.compute_cgi(mine, start[q + 1] - start[q], q, frag_len)
        cell = pc.cells(b, mine)
        assert rc.same_rows(pc.rows_of(b, cell, start[q + 1] - start[q], q), rows), (name, frag_len, q)
        for key, edges in edge_sets(cell).items():
            rec, hist = expected(b, rows, lambda qid: cell, edges)
            assert len(rec) == len(rows) and np.array_equal(rec["count"], rows["countSeq"].astype(np.uint32)), (name, key)
            assert np.array_equal(hist.sum(axis=1), rows["countSeq"]) and hist.shape[1] == len(edges) + 1
            st = np.stack([bits(rec[f]) for f in ("minIdentity", "q1", "median", "q3", "maxIdentity")], axis=1).astype(np.int64)
            assert (np.diff(st, axis=1) >= 0).all()
            n_rec += len(rec)
    assert n_rec >= 1
    if name in ("c2", "c3", "c4", "c5", "c8"):
        want = {"c2": 2, "c3": 3, "c4": 4, "c5": 5, "c8": 8}[name]
        rows = osk.compute_cgi(maps, frags, 0, frag_len)
        assert int(rows["countSeq"][rows["refGenomeId"] == rc.G63][0]) == want


# ---- one query: ani_compute_cgi ----
def one_gates(rows):
    """no gate; and, where the rows allow it, the upper median of the identities and of countSeq (a row's own value: on the threshold)"""
    gates = [(0.0, 1)]
    if len(rows) >= 2:
        gates.append((np.sort(rows["identity"])[len(rows) // 2], 1))
        gates.append((0.0, int(np.sort(rows["countSeq"])[len(rows) // 2])))
    return gates


def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    exp_rows = ref.expected(maps, frags, 4)
    cell = pc.cells(b, maps)
    sets = edge_sets(cell)
    exp_open = {}
    for key, edges in sets.items():
        for gate in one_gates(exp_rows):
            exp = expected(b, exp_rows, lambda qid: cell, edges, gate)
            if gate == (0.0, 1):
                exp_open[key] = exp
                assert len(exp[0]) == len(exp_rows)
            for order in ((rc.in_order, rc.shuffled) if key in ("default", "on_cell") else (rc.in_order,)):
                sk.fragdist_begin(edges, *gate)
                got_rows = sk.compute_cgi(order(maps), frags, 4)
                got = sk.fragdist_take()
                sk.fragdist_end()
                what = "%s, fragLen %d, edges %s, gate %r, %s" % (name, lay.frag_len, key, gate, order.__name__)
                assert rc.same_rows(got_rows, exp_rows), what
                assert same(got, exp, what)
    check_edge_sets(name, sets, exp_open, cell)
    rec = exp_open["none"][0]
    if name == "dense":
        assert sorted(int(c) for c in rec["count"]) == [65, 129]
    if name == "n1":
        assert len(rec) == 1 and int(rec["count"][0]) == 1 and len(set(bits(rec[f])[0] for f in ("minIdentity", "q1", "median", "q3", "maxIdentity"))) == 1
    if name == "n0":
        assert len(rec) == 0


def case_slab_edge(ref):
    """exactly 64 and 65 values: every bin of the 64- and the 65-bin genome"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    r = rc.rng(34, lay.frag_len)
    c, pos = [], []
    for g in (rc.G64, rc.G65):
        for x, j in lay.genome_bins(g):
            c.append(x)
            pos.append(lay.pos_in_bin(x, j, r))
    maps = rc.mappings(lay, r.permutation(len(c)), c, pos, rc.full_mantissa(r, len(c)))
    rows = ref.expected(maps, len(c), 0)
    assert sorted(int(x) for x in rows["countSeq"]) == [64, 65]
    cell = pc.cells(b, maps)
    for edges in ((), DEFAULT_EDGES):
        sk.fragdist_begin(edges)
        assert rc.same_rows(sk.compute_cgi(maps, len(c), 0), rows)
        assert same(sk.fragdist_take(), expected(b, rows, lambda qid: cell, edges), "slab edge")
        sk.fragdist_end()


# ---- several queries in one table: ani_reduce_check ----
def cells_many(b, maps, start, first_id):
    out = {}
    for q in range(len(start) - 1):
        out[first_id + q] = pc.cells(b, maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])])
    return out


def case_many(ref, name, gated=False):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps0, frags = LISTS[name](lay)
    all_cells = pc.cells(b, maps0)
    sets = edge_sets(all_cells)
    keys = ("default", "on_cell", "none", "max63")
    run = 0
    for n_query in ((3, 5) if gated else (1, 2, 5)):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (3, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                gate = pc.oracle_gate(ref, maps, start) if gated else (0.0, 1)
                exp_rows = rc.expected_many(ref, maps, start, 7)
                cm = cells_many(b, maps, start, 7)
                key = keys[run % len(keys)]
                run += 1
                exp = expected(b, exp_rows, cm.__getitem__, sets[key], gate)
                assert (0 < len(exp[0]) < len(exp_rows)) if gated else len(exp[0]) == len(exp_rows)
                for order in (rc.in_order, rc.shuffled):
                    sk.fragdist_begin(sets[key], *gate)
                    got_rows = rc.reduce_check(ref, order(maps), start, genome_base, 7)
                    got = sk.fragdist_take()
                    sk.fragdist_end()
                    what = "%s, fragLen %d, %d queries %r, genomeBase %d, edges %s, gate %r, %s" % (name, lay.frag_len, n_query, start, genome_base, key, gate,
                                                                                                order.__name__)
                    assert rc.same_rows(got_rows, exp_rows), what
                    assert same(got, exp, what)


def case_gate_edges(ref):
    """the gate's own edges on `random` over 5 queries, as profile_cases.case_gate_edges: -0.0 is 0; a row on the identity threshold
    contributes and the next float above it shuts it out; countSeq = minFragments contributes and minFragments - 1 does not"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_random(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    cm = cells_many(b, maps, start, 0)
    thr = np.sort(rows["identity"])[len(rows) // 2]
    above = np.nextafter(thr, np.float32(200.0))
    below = np.nextafter(thr, np.float32(0.0))
    n_at = int((bits(rows["identity"]) >= bits(thr)).sum())
    n_above = int((bits(rows["identity"]) >= bits(above)).sum())
    assert n_at > n_above > 0
    top = int(rows["countSeq"].max())
    n_top = int((rows["countSeq"] == top).sum())
    for gate, n in (((-0.0, 1), len(rows)), ((thr, 1), n_at), ((below, 1), n_at), ((above, 1), n_above), ((100.0, 1), 0), ((0.0, top + 1), 0), ((0.0, top), n_top)):
        sk.fragdist_begin(DEFAULT_EDGES, *gate)
        got_rows = rc.reduce_check(ref, maps, start, 0, 0)
        got = sk.fragdist_take()
        sk.fragdist_end()
        assert rc.same_rows(got_rows, rows), gate
        assert len(got[0]) == n, (gate, len(got[0]), n)
        assert same(got, expected(b, rows, cm.__getitem__, DEFAULT_EDGES, gate), repr(gate))


# ---- life cycle and arguments ----
def expect_error(fn, what, code=ERR_ARG):
    return pc.expect_error(fn, what, code)


def case_life_cycle(ref):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    a_maps, a_frags = rc.list_random(lay)
    b_maps, b_frags = rc.list_ties(lay)
    a_maps = rc.in_order(a_maps)
    a_rows = ref.expected(a_maps, a_frags, 1)
    start = rc.split_queries(b_frags, 5, 5)
    many_rows = rc.expected_many(ref, b_maps, start, 10)
    a_cell, b_cells = pc.cells(b, a_maps), cells_many(b, b_maps, start, 10)
    edges = DEFAULT_EDGES
    exp_a = expected(b, a_rows, lambda qid: a_cell, edges)
    exp_b = expected(b, many_rows, b_cells.__getitem__, edges)
    both = (np.concatenate([exp_a[0], exp_b[0]]), np.concatenate([exp_a[1], exp_b[1]]))

    # rows with the mode off, as the reference of rule 7
    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    assert rc.same_rows(off_a, a_rows) and rc.same_rows(off_b, many_rows)

    # two calls, one take: call order; the second take is empty
    sk.fragdist_begin(edges)
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.fragdist_take(), both, "two calls")
    empty = sk.fragdist_take()
    assert empty[0].shape == (0,) and empty[1].shape == (0, len(edges) + 1)
    # a take between two calls: the union is the whole, in order
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.fragdist_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    second = sk.fragdist_take()
    assert same(first, exp_a) and same(second, exp_b)
    # ani_map_query adds nothing (on the layout's own sequences: the engine has an index to map against)
    # begin twice: the second drops what is pending and takes the new gate and edges
    sk.compute_cgi(a_maps, a_frags, 1)
    gate = pc.oracle_gate(ref, b_maps, start)
    sk.fragdist_begin((90.0,), *gate)
    rc.reduce_check(ref, b_maps, start, 0, 10)
    exp_gated = expected(b, many_rows, b_cells.__getitem__, (90.0,), gate)
    assert 0 < len(exp_gated[0]) < len(many_rows)
    assert same(sk.fragdist_take(), exp_gated, "second begin")
    # the C call with hist = NULL, and n = 0 gives NULL pointers
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    rp, hp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_fragdist_take(sk.h, ctypes.byref(rp), None, ctypes.byref(n)))
    assert n.value == len(exp_gated[0]) and rp.value
    raw = ctypes.string_at(rp.value, n.value * FRAGDIST_DT.itemsize)
    lib.ani_free(rp)
    assert raw == exp_gated[0].tobytes()
    rp, hp, n = ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_size_t(5)
    chk(lib.ani_sketch_fragdist_take(sk.h, ctypes.byref(rp), ctypes.byref(hp), ctypes.byref(n)))
    assert n.value == 0 and not rp.value and not hp.value
    # end: take and end are refused, mapping works and returns the same rows
    rc.reduce_check(ref, b_maps, start, 0, 10)               # pending records go with end
    sk.fragdist_end()
    expect_error(sk.fragdist_take, "take after end")
    expect_error(sk.fragdist_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.fragdist_begin(edges)
    assert len(sk.fragdist_take()[0]) == 0                   # nothing of before the end
    sk.fragdist_end()


def case_with_profile(ref):
    """the profile and the distribution on together: both right, rows equal"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    p_gate, d_gate = pc.oracle_gate(ref, maps, start), (0.0, int(np.sort(rows["countSeq"])[len(rows) // 3]))
    sk.profile_begin(*p_gate)
    sk.fragdist_begin(DEFAULT_EDGES, *d_gate)
    got_rows = rc.reduce_check(ref, maps, start, 0, 0)
    assert rc.same_rows(got_rows, rows)
    assert pc.same_profile(sk.profile_read(), pc.Profile(b, *p_gate).add_many(maps, start))
    exp = expected(b, rows, cells_many(b, maps, start, 0).__getitem__, DEFAULT_EDGES, d_gate)
    assert 0 < len(exp[0]) < len(rows)
    assert same(sk.fragdist_take(), exp, "with the profile on")
    sk.profile_end()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.fragdist_take(), exp, "after the profile's end")
    sk.fragdist_end()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    f32 = np.float32
    expect_error(sk.fragdist_take, "take without begin")
    expect_error(sk.fragdist_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.fragdist_begin((), v, 1), "minIdentity " + what)
        expect_error(lambda: sk.fragdist_begin((50.0, v), 0.0, 1), "an edge " + what)
        expect_error(lambda: sk.fragdist_begin((v,), 0.0, 1), "a first edge " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.fragdist_begin((), 50.0, n), "minFragments %d" % n)
    expect_error(lambda: sk.fragdist_begin((80.0, 80.0)), "equal edges")
    expect_error(lambda: sk.fragdist_begin((80.0, 79.0)), "descending edges")
    expect_error(lambda: sk.fragdist_begin((0.0, -0.0)), "0 after 0")
    expect_error(lambda: sk.fragdist_begin(np.linspace(1.0, 99.0, 64)), "64 edges")
    expect_error(sk.fragdist_take, "take after a refused begin")
    one = (ctypes.c_float * 1)(90.0)
    expect_error(lambda: chk(lib.ani_sketch_fragdist_begin(None, 0.0, 1, None, 0)), "begin(null)")
    expect_error(lambda: chk(lib.ani_sketch_fragdist_begin(sk.h, 0.0, 1, None, 1)), "null edges with nEdges 1")
    expect_error(lambda: chk(lib.ani_sketch_fragdist_begin(sk.h, 0.0, 1, one, -1)), "nEdges -1")
    expect_error(lambda: chk(lib.ani_sketch_fragdist_begin(sk.h, 0.0, 1, one, 64)), "nEdges 64")
    rp, hp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    expect_error(lambda: chk(lib.ani_sketch_fragdist_take(None, ctypes.byref(rp), ctypes.byref(hp), ctypes.byref(n))), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_fragdist_end(None)), "end(null)")
    # a refused begin leaves a running distribution, its gate and its edges alone
    sk.fragdist_begin((90.0,), 0.0, 1)
    rows = sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: sk.fragdist_begin((), 101.0, 1), "minIdentity 101")
    expect_error(lambda: sk.fragdist_begin((101.0,)), "edge 101")
    expect_error(lambda: chk(lib.ani_sketch_fragdist_take(sk.h, None, None, ctypes.byref(n))), "take(sk, null)")
    rec, hist = sk.fragdist_take()
    assert len(rec) == len(rows) and hist.shape == (len(rows), 2)
    # the limits of the ranges are accepted
    sk.fragdist_begin((0.0, 100.0), 100.0, 2 ** 31 - 1)
    sk.fragdist_begin(np.linspace(0.0, 100.0, 63), -0.0, 1)
    sk.fragdist_begin(())
    sk.fragdist_end()


# ---- end to end: the mapper's own cells ----
E2E_GATE = pc.E2E_GATE


class EndToEnd:
    """the inputs of profile_cases.e2e_genomes, each query's ani_map_query mappings and their cells and rows, made once per half by the
    default engine"""

    def __init__(self, engine):
        self.refs, self.queries = pc.e2e_genomes()
        self.p = engine.params(pc.E2E_K, pc.E2E_FRAG_LEN)
        sk = Sketch(engine, self.p, self.refs)
        self.n_minimizers = sk.stats()["minimizers"]
        contig_len = [len(c) for g in self.refs for c in g]
        contig_genome = [g for g, cs in enumerate(self.refs) for _ in cs]
        self.b = pc.Bins(contig_len, contig_genome, pc.E2E_FRAG_LEN)
        self.cells, rows = {}, []
        sk.fragdist_begin(DEFAULT_EDGES)
        for qi, q in enumerate(self.queries):
            maps, total = sk.map_query(q)
            assert len(sk.fragdist_take()[0]) == 0            # ani_map_query adds nothing
            self.cells[qi] = pc.cells(self.b, maps)
            sk.fragdist_end()
            rows.append(sk.compute_cgi(maps, total, qi))
            sk.fragdist_begin(DEFAULT_EDGES)
        sk.close()                                          # destroyed with the mode on
        self.rows = np.concatenate(rows)
        self.open = self.expect(self.rows, (0.0, 1))
        self.gated = self.expect(self.rows, E2E_GATE)
        assert 0 < len(self.gated[0]) < len(self.open[0]) == len(self.rows)
        assert int(self.open[0]["count"].max()) > 40 and int(self.open[0]["count"].min()) < 10
        assert (bits(self.open[0]["q1"]) < bits(self.open[0]["q3"])).any()

    def expect(self, rows, gate, ref_base=0):
        return expected(self.b, rows, self.cells.__getitem__, DEFAULT_EDGES, gate, ref_base)

    def run(self, engine, config):
        sk = Sketch(engine, self.p, self.refs)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        sets = [engine.fragment_set(self.p, self.queries[:3]), engine.fragment_set(self.p, self.queries[3:])]
        off_rows = sk.map_cgi_batch(self.queries, 0)
        assert rc.same_rows(off_rows, self.rows), config
        for gate, exp in ((E2E_GATE, self.gated), ((0.0, 1), self.open)):
            sk.fragdist_begin(DEFAULT_EDGES, *gate)
            rows = sk.map_cgi_batch(self.queries, 0)
            assert rc.same_rows(rows, self.rows), config
            assert same(sk.fragdist_take(), exp, config + ", map_cgi_batch, gate %r" % (gate,))
            rows = sk.map_cgi_fragsets(sets, [0, 3])
            assert rc.same_rows(rows, self.rows), config
            assert same(sk.fragdist_take(), exp, config + ", map_cgi_fragsets, gate %r" % (gate,))
        # a reference id base, and query ids that do not start at 0: the records carry the rows' ids
        sk.set_ref_id_base(500)
        moved = self.rows.copy()
        moved["refGenomeId"] += 500
        moved["qryGenomeId"] += 20
        cells = dict((q + 20, c) for q, c in self.cells.items())
        exp = expected(self.b, moved, cells.__getitem__, DEFAULT_EDGES, E2E_GATE, 500)
        sk.fragdist_begin(DEFAULT_EDGES, *E2E_GATE)
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 20), moved), config
        assert same(sk.fragdist_take(), exp, config + ", id base, map_cgi_batch")
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [20, 23]), moved), config
        assert same(sk.fragdist_take(), exp, config + ", id base, map_cgi_fragsets")
        for s in sets:
            s.close()
        sk.close()                                          # a sketch destroyed with the mode on releases its list


# ---- the command line: --fragDist ----
def fmt(x):
    return "%g" % float(x)


def fragdist_lines(out_lines, q_paths, r_paths, edges, rec, hist):
    """the .fragdist file for the lines of the -o file, from the Python API's records of one sketch over all references (query and
    reference ids = list positions)"""
    at = dict(((int(r["qryGenomeId"]), int(r["refGenomeId"])), i) for i, r in enumerate(rec))
    qi, ri = dict((p, i) for i, p in enumerate(q_paths)), dict((p, i) for i, p in enumerate(r_paths))
    out = ["#edges\t" + ",".join(fmt(np.float32(e)) for e in edges)]
    for line in out_lines:
        q, r = line.split("\t")[:2]
        i = at.get((qi[q], ri[r]))
        if i is None:
            continue
        x = rec[i]
        out.append("\t".join([q, r, str(int(x["count"]))] + [fmt(x[f]) for f in ("minIdentity", "q1", "median", "q3", "maxIdentity")]
                             + [",".join(str(int(h)) for h in hist[i])]))
    return out


def case_cli(binary, engine, tmp, mode):
    import os
    import subprocess
    all_vs_all, extra = pc.CLI_MODES[mode]
    refs, queries = pc.e2e_genomes(pc.CLI_LEN)
    if all_vs_all:
        refs = queries = refs + queries[:2]
    files = {}

    def write(kind, genomes):
        paths = []
        for i, g in enumerate(genomes):
            key = id(g)
            if key not in files:
                files[key] = os.path.join(tmp, "%s%d.fa" % (kind, i))
                rc.orc.write_fasta(files[key], g, names=["%s%d_%d" % (kind, i, j) for j in range(len(g))])
            paths.append(files[key])
        lst = os.path.join(tmp, kind + ".txt")
        open(lst, "w").write("\n".join(paths) + "\n")
        return paths, lst

    r_paths, rl = write("r", refs)
    q_paths, ql = write("q", queries)
    base = [binary, "--ql", ql, "--rl", rl, "--fragLen", str(pc.E2E_FRAG_LEN), "-k", str(pc.E2E_K), "--matrix"] + extra
    plain, dist = os.path.join(tmp, "plain.out"), os.path.join(tmp, "dist.out")
    p = engine.params(pc.E2E_K, pc.E2E_FRAG_LEN)

    def api(edges, gate):
        sk = Sketch(engine, p, refs)
        sk.fragdist_begin(edges, *gate)
        sk.map_cgi_batch(queries, 0)
        got = sk.fragdist_take()
        sk.close()
        return got

    def run(out, opts):
        r = subprocess.run(base + ["-o", out] + opts, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]

    run(plain, [])
    # the default edges and gate: a line for every -o line; every other file is what it was
    run(dist, ["--fragDist"])
    produced = sorted(f[len("plain.out"):] for f in os.listdir(tmp) if f.startswith("plain.out"))
    assert produced == ["", ".matrix"] and sorted(f[len("dist.out"):] for f in os.listdir(tmp) if f.startswith("dist.out")) == ["", ".fragdist", ".matrix"]
    for suffix in produced:
        assert open(plain + suffix, "rb").read() == open(dist + suffix, "rb").read(), suffix
    out_lines = open(plain).read().splitlines()
    assert len(out_lines) >= 6
    rec, hist = api(DEFAULT_EDGES, (0.0, 1))
    got = open(dist + ".fragdist").read().splitlines()
    exp = fragdist_lines(out_lines, q_paths, r_paths, DEFAULT_EDGES, rec, hist)
    assert got == exp, "%s: %d lines, expected %d; first difference %r" % (mode, len(got), len(exp), next(((a, b) for a, b in zip(got, exp) if a != b), None))
    assert len(got) == len(out_lines) + 1 and got[0] == "#edges\t" + ",".join(str(e) for e in range(70, 100)) + ",99.5,99.9"
    if mode == "lists":
        # lines of -o that --minFraction drops have no line here: the records are joined on (query, reference)
        strict, strict_dist = os.path.join(tmp, "strict.out"), os.path.join(tmp, "strict_dist.out")
        run(strict, ["--minFraction", "0.9"])
        run(strict_dist, ["--minFraction", "0.9", "--fragDist"])
        strict_lines = open(strict).read().splitlines()
        assert 0 < len(strict_lines) < len(out_lines) and open(strict_dist).read().splitlines() == strict_lines
        assert open(strict_dist + ".fragdist").read().splitlines() == fragdist_lines(strict_lines, q_paths, r_paths, DEFAULT_EDGES, rec, hist)
    # a gate that drops the record of at least one -o line and keeps at least one; edges of the caller's
    edges = (80.0, 95.0, 99.0)
    ids = sorted(set(float(line.split("\t")[2]) for line in out_lines))
    assert ids[-1] - ids[0] > 0.01
    gate = (float("%.4f" % ((ids[0] + ids[-1]) / 2)), 2)      # between the lowest and the highest ANI of the -o lines
    run(dist, ["--fragDist", "--fragDistEdges", "80,95,99", "--fragDistMinANI", str(gate[0]), "--fragDistMinFragments", str(gate[1])])
    for suffix in produced:
        assert open(plain + suffix, "rb").read() == open(dist + suffix, "rb").read(), suffix
    rec, hist = api(edges, gate)
    got = open(dist + ".fragdist").read().splitlines()
    assert got == fragdist_lines(out_lines, q_paths, r_paths, edges, rec, hist), mode
    assert 1 < len(got) < len(out_lines) + 1, (len(got), len(out_lines))
    if mode == "lists":
        # with --profile and --visualize beside it
        for opts, more in ((["--profile"], [".profile"]), (["--visualize"], [".visual"])):
            both = os.path.join(tmp, "both%s.out" % more[0])
            run(both, ["--fragDist", "--fragDistEdges", "80,95,99", "--fragDistMinANI", str(gate[0]), "--fragDistMinFragments", str(gate[1])] + opts)
            assert open(both + ".fragdist").read().splitlines() == got, opts
            assert open(both, "rb").read() == open(plain, "rb").read() and os.path.exists(both + more[0])
        # the dependent options are refused by name without --fragDist, and bad values before anything is mapped
        for opts, msg in ((["--fragDistEdges", "90"], b"--fragDistEdges needs --fragDist"), (["--fragDistMinANI", "90"], b"--fragDistMinANI needs --fragDist"),
                          (["--fragDistMinFragments", "5"], b"--fragDistMinFragments needs --fragDist"),
                          (["--fragDist", "--fragDistMinANI", "-1"], b"--fragDistMinANI takes"), (["--fragDist", "--fragDistMinANI", "100.5"], b"--fragDistMinANI takes"),
                          (["--fragDist", "--fragDistMinFragments", "0"], b"--fragDistMinFragments takes"),
                          (["--fragDist", "--fragDistEdges", "90,90"], b"--fragDistEdges takes"), (["--fragDist", "--fragDistEdges", "90,x"], b"--fragDistEdges takes"),
                          (["--fragDist", "--fragDistEdges", "90,101"], b"--fragDistEdges takes"), (["--fragDist", "--fragDistEdges", "nan"], b"--fragDistEdges takes"),
                          (["--fragDist", "--fragDistEdges", ",".join(str(i) for i in range(1, 65))], b"--fragDistEdges takes")):
            r = subprocess.run(base + ["-o", os.path.join(tmp, "refused.out")] + opts, capture_output=True)
            assert r.returncode == 1 and msg in r.stderr, (opts, r.stderr[-500:])
        assert not os.path.exists(os.path.join(tmp, "refused.out"))
