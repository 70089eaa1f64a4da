"""Cases for the percentile bootstrap intervals of the ANI values (kernels/ci.hpp: k_ci_flags, k_ci_list, k_ci_records; ci_stage,
collect_rows and ani_sketch_ci_begin / _take / _end in engine_map.hip), shared by the GPU tests (-m gpu, product library) and the
CPU-emulation tests (not gpu, tests/emu build): test_ci.py.

The reference is a numpy restatement of rules 1 - 5 of include/ani_abi.h over the cells of profile_cases.py (themselves held to the
oracle's rows there): per row that passes the gate, the genome's non-empty cells in bin order, fix of each, the draws of the stated
hash, the replicate sums and the two order statistics by a sort.  The ids and the order of the expected records are those of the rows
the same call returned.  Every comparison is on bits; there is no tolerance.  The statistical check of the restatement (a hash that is
not uniform must not slip through) is the only place with a band, the issue's [0.85, 1.15].

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins) and the engines are those of reduce_cases.py
and fragdist_cases.py."""
import ctypes

import numpy as np

import fragdist_cases as fc
import hits_cases as hc
import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import CI_DT, Sketch

ERR_ARG = rc.ERR_ARG
FIX = pc.FIX
bits = pc.bits
LISTS = fc.LISTS
LISTS_ONE = fc.LISTS_ONE
LISTS_MANY = fc.LISTS_MANY
LISTS_GATE = fc.LISTS_GATE
LISTS_RESTATE = ("random", "ties", "dense", "c2", "c3", "c5", "low_bits", "all_equal", "n1")
B_ONE = 16                                              # replicates of the engine tests (the emulation build keeps B <= 64)
SWEEP_B = (1, 2, 7, 64, 65, 200, 1024)
SWEEP_L = (1, 500, 950, 999)
M32 = np.uint64(0xffffffff)


# ---- rules 1 - 4 ----
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


_idx = {}


def draws(count, replicates, seed):
    """idx[r, j] of rule 3: uint64[replicates, count]; they depend on (seed, r, j, count) only, so they are kept"""
    key = (int(count), int(replicates), int(seed))
    if key not in _idx:
        if len(_idx) > 64:
            _idx.clear()
        r = np.arange(1, replicates + 1, dtype=np.uint64)
        j = np.arange(1, count + 1, dtype=np.uint64)
        k = fmix32((np.uint64(seed) + np.uint64(0x9e3779b9) * r) & M32)
        u = fmix32(k[:, None] ^ ((np.uint64(0x85ebca6b) * j) & M32)[None, :])
        _idx[key] = (u * np.uint64(count)) >> np.uint64(32)
    return _idx[key]


def fix(v):
    """F of rule 1 for the bit patterns v"""
    return np.rint(np.asarray(v, dtype=np.uint32).view(np.float32).astype(np.float64) * FIX).astype(np.uint64)


def ranks(replicates, permille):
    low = ((replicates - 1) * (1000 - permille)) // 2000
    return low, replicates - 1 - low


def interval(f, replicates, permille, seed):
    """F in bin order -> (sum, lowSum, highSum): the definition, no shortcut"""
    f = np.asarray(f, dtype=np.uint64)
    s = np.sort(f[draws(len(f), replicates, seed)].sum(axis=1, dtype=np.uint64))
    lo, hi = ranks(replicates, permille)
    return int(f.sum(dtype=np.uint64)), int(s[lo]), int(s[hi])


def bound(total, count):
    return np.float32(np.float64(total) / (np.float64(count) * FIX))


def expected(b, rows, cell_of, replicates=B_ONE, permille=950, seed=1, gate=(0.0, 1), ref_base=0):
    """the records of the pairs of `rows` (the rows a call returned, in its order) that pass the gate; cell_of(qryGenomeId) = that
    query's cells (profile_cases.cells); a row's genome is refGenomeId - ref_base"""
    min_bits, min_frag = pc.gate_bits(gate[0]), int(gate[1])
    rec = []
    for row in rows:
        if int(row["countSeq"]) < min_frag or int(bits(row["identity"])) < min_bits:
            continue
        g = int(row["refGenomeId"]) - ref_base
        cell = cell_of(int(row["qryGenomeId"]))[int(b.genome_start[g]):int(b.genome_start[g + 1])]
        v = cell[cell != 0]                                 # bin order
        assert len(v) == int(row["countSeq"])               # rule 1
        total, low, high = interval(fix(v), replicates, permille, seed)
        r = np.zeros(1, dtype=CI_DT)
        r["refGenomeId"], r["qryGenomeId"], r["count"], r["replicates"] = row["refGenomeId"], row["qryGenomeId"], len(v), replicates
        r["sum"], r["lowSum"], r["highSum"] = total, low, high
        r["low"], r["high"] = bound(low, len(v)), bound(high, len(v))
        rec.append(r)
    return np.concatenate(rec) if rec else np.zeros(0, dtype=CI_DT)


def same(got, exp, what=""):
    assert got.dtype == CI_DT, got.dtype
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != exp[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, the first at %d:\n%r\n%r" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]]))
    return True


def run_one(sk, maps, frags, qid, **kw):
    sk.ci_begin(**kw)
    rows = sk.compute_cgi(maps, frags, qid)
    got = sk.ci_take()
    sk.ci_end()
    return rows, got


def begin_args(replicates=B_ONE, permille=950, seed=1, gate=(0.0, 1)):
    return dict(replicates=replicates, level=permille / 10.0, seed=seed, min_identity=gate[0], min_fragments=gate[1])


# ---- the restatement against the oracle and against statistics: CPU only, no engine ----
def case_restatement(frag_len, name):
    lay = rc.Layout(frag_len)
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    osk = pc.oracle_sketch(frag_len)
    start = rc.split_queries(frags, 3, 3) if frags > 3 else [0, frags]
    n_rec = 0
    for q in range(len(start) - 1):
        mine = maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])] if frags > 3 else maps   # (n1: one mapping, any id)
        rows = osk.compute_cgi(mine, start[q + 1] - start[q], q, frag_len)
        cell = pc.cells(b, mine)
        # count, and the cell order: the cells added in float in bin order and divided by the count are the oracle's identity, bit for
        # bit (the hits' rule 5)
        assert rc.same_rows(pc.rows_of(b, cell, start[q + 1] - start[q], q), rows), (name, frag_len, q)
        for replicates, permille in ((B_ONE, 950), (200, 950), (7, 500)):
            rec = expected(b, rows, lambda qid: cell, replicates, permille)
            assert len(rec) == len(rows) and np.array_equal(rec["count"], rows["countSeq"].astype(np.uint32)), name
            assert (rec["lowSum"] <= rec["highSum"]).all() and (rec["replicates"] == replicates).all()
            # a replicate sum lies between count times the smallest and count times the largest F
            for r, row in zip(rec, rows):
                g = int(row["refGenomeId"])
                v = cell[int(b.genome_start[g]):int(b.genome_start[g + 1])]
                f = fix(v[v != 0])
                assert int(f.min()) * len(f) <= int(r["lowSum"]) and int(r["highSum"]) <= int(f.max()) * len(f)
                if int(f.min()) == int(f.max()):
                    assert int(r["lowSum"]) == int(r["highSum"]) == int(r["sum"])
            n_rec += len(rec)
    assert n_rec >= 1
    if name in ("all_equal", "n1"):
        rows = osk.compute_cgi(maps, frags, 0, frag_len)
        rec = expected(b, rows, lambda qid: pc.cells(b, maps))
        assert (rec["lowSum"] == rec["sum"]).all() and (rec["highSum"] == rec["sum"]).all() and (bits(rec["low"]) == bits(rec["high"])).all()
    if name == "n1":
        assert len(rec) == 1 and int(rec["count"][0]) == 1


STAT_N = (64, 300, 1678)
STAT_SEEDS = range(20)


def stat_cells(kind, n):
    r = rc.rng(41, n, 0 if kind == "uniform" else 1)
    if kind == "uniform":
        x = r.uniform(80.0, 100.0, n)
    else:
        x = np.where(r.random(n) < 0.3, r.uniform(80.0, 85.0, n), r.uniform(97.0, 100.0, n))
    return x.astype(np.float32)


def case_statistics(kind, n):
    """B = 1000, L = 950, seeds 0..19: every interval brackets the sum, and its width over the normal approximation's lies in
    [0.85, 1.15] (the issue's band; the rules as stated gave 0.897 .. 1.074 there)"""
    x = stat_cells(kind, n)
    f = fix(bits(x))
    sd = float(np.std(x.astype(np.float64), ddof=1))
    ratios = []
    for seed in STAT_SEEDS:
        total, low, high = interval(f, 1000, 950, seed)
        assert low <= total <= high, (kind, n, seed, low, total, high)
        ratios.append(float(np.float64(bound(high, n)) - np.float64(bound(low, n))) / (2 * 1.96 * sd / np.sqrt(n)))
    print("%s n=%d: width ratio %.3f .. %.3f" % (kind, n, min(ratios), max(ratios)))
    assert 0.85 <= min(ratios) and max(ratios) <= 1.15, (kind, n, min(ratios), max(ratios))


def case_uniform_positions():
    """the positions themselves: chi^2 / df of the draws over the cells near 1, and successive replicates uncorrelated"""
    for count in (64, 300, 1678):
        chi, df = 0.0, 0
        for seed in range(5):
            idx = draws(count, 1000, seed)
            c = np.bincount(idx.reshape(-1).astype(np.int64), minlength=count).astype(np.float64)
            e = idx.size / count
            chi += float(((c - e) ** 2 / e).sum())
            df += count - 1
        assert abs(chi / df - 1.0) < 4.0 * np.sqrt(2.0 / df), (count, chi / df)       # four standard deviations of chi^2 / df
    f = fix(bits(stat_cells("uniform", 300))).astype(np.float64)
    cor = []
    for seed in range(30):
        s = f[draws(300, 1000, seed)].sum(axis=1)
        cor.append(float(np.corrcoef(s[:-1], s[1:])[0, 1]))
    assert abs(float(np.mean(cor))) < 4 * 0.032 / np.sqrt(30) + 0.01, np.mean(cor)     # 1 / sqrt(999) a seed


# ---- one query: ani_compute_cgi ----
def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    exp_rows = ref.expected(maps, frags, 4)
    cell = pc.cells(b, maps)
    for gate in fc.one_gates(exp_rows):
        exp = expected(b, exp_rows, lambda qid: cell, gate=gate)
        for order in (rc.in_order, rc.shuffled):
            got_rows, got = run_one(sk, order(maps), frags, 4, **begin_args(gate=gate))
            what = "%s, fragLen %d, gate %r, %s" % (name, lay.frag_len, gate, order.__name__)
            assert rc.same_rows(got_rows, exp_rows), what
            assert same(got, exp, what)
        if gate == (0.0, 1):
            assert len(exp) == len(exp_rows)
            if name == "dense":
                assert sorted(int(c) for c in exp["count"]) == [65, 129] and (exp["lowSum"] < exp["highSum"]).all()
            if name == "n1":
                assert len(exp) == 1 and int(exp["count"][0]) == 1
            if name == "n0":
                assert len(exp) == 0
            if name == "all_equal":
                assert (exp["lowSum"] == exp["highSum"]).all()


def case_sweep(ref, replicates):
    """`dense` (129 and 65 cells): every level at `replicates`; ranks 0 and B - 1, and lowRank = highRank at B = 1"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = LISTS["dense"](lay)
    rows = ref.expected(maps, frags, 0)
    cell = pc.cells(b, maps)
    seen = set()
    for permille in SWEEP_L:
        seen.add(ranks(replicates, permille))
        exp = expected(b, rows, lambda qid: cell, replicates, permille)
        got_rows, got = run_one(sk, maps, frags, 0, **begin_args(replicates, permille))
        assert rc.same_rows(got_rows, rows) and same(got, exp, "B %d, L %d" % (replicates, permille))
    assert all(lo <= hi and lo + hi == replicates - 1 for lo, hi in seen)
    assert ranks(replicates, 999) == (0, replicates - 1) and ranks(replicates, 1)[0] == ((replicates - 1) * 999) // 2000
    if replicates == 1:
        assert seen == {(0, 0)}


# ---- several queries in one table: ani_reduce_check ----
cells_many = fc.cells_many


def many_runs(maps0, frags, gated):
    """the (maps, start, genome_base) of fragdist_cases.case_many"""
    for n_query in ((3, 5) if gated else (1, 2, 5)):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (3, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                yield maps, start, genome_base


def case_many(ref, name, gated=False, also=None):
    """`also`: a second Ref (the default engine's) whose records must equal this one's"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps0, frags = LISTS[name](lay)
    for maps, start, genome_base in many_runs(maps0, frags, gated):
        gate = pc.oracle_gate(ref, maps, start) if gated else (0.0, 1)
        exp_rows = rc.expected_many(ref, maps, start, 7)
        exp = expected(b, exp_rows, cells_many(b, maps, start, 7).__getitem__, gate=gate)
        assert (0 < len(exp) < len(exp_rows)) if gated else len(exp) == len(exp_rows)
        for order in (rc.in_order, rc.shuffled):
            what = "%s, fragLen %d, queries %r, genomeBase %d, gate %r, %s" % (name, lay.frag_len, start, genome_base, gate, order.__name__)
            for r in (ref,) if also is None else (ref, also):
                r.sk.ci_begin(**begin_args(gate=gate))
                got_rows = rc.reduce_check(r, order(maps), start, genome_base, 7)
                got = r.sk.ci_take()
                r.sk.ci_end()
                assert rc.same_rows(got_rows, exp_rows), what
                assert same(got, exp, what)


def case_gate_edges(ref):
    """the gate's own edges on `random` over 5 queries, as fragdist_cases.case_gate_edges"""
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
        sk.ci_begin(**begin_args(gate=gate))
        got_rows = rc.reduce_check(ref, maps, start, 0, 0)
        got = sk.ci_take()
        sk.ci_end()
        assert rc.same_rows(got_rows, rows), gate
        assert len(got) == n, (gate, len(got), n)
        assert same(got, expected(b, rows, cm.__getitem__, gate=gate), repr(gate))


def case_seeds(ref):
    """two seeds give different lowSum on `random`; the same seed twice gives equal records"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_random(lay)
    rows = ref.expected(maps, frags, 0)
    cell = pc.cells(b, maps)
    got = {}
    for seed in (1, 2, 1, 0, 0xffffffff):
        _, rec = run_one(sk, maps, frags, 0, **begin_args(seed=seed))
        assert same(rec, expected(b, rows, lambda qid: cell, seed=seed), "seed %d" % seed)
        if seed in got:
            assert rec.tobytes() == got[seed].tobytes()
        got[seed] = rec
    assert (got[1]["lowSum"] != got[2]["lowSum"]).any() and np.array_equal(got[1]["sum"], got[2]["sum"])


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
    a_cell, b_cells = pc.cells(b, a_maps), cells_many(b, b_maps, start, 10)
    exp_a = expected(b, a_rows, lambda qid: a_cell)
    exp_b = expected(b, many_rows, b_cells.__getitem__)
    arg = begin_args()

    # rows with the mode off, as the reference of rule 6
    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    assert rc.same_rows(off_a, a_rows) and rc.same_rows(off_b, many_rows)
    # two calls, one take: call order; the second take is empty
    sk.ci_begin(**arg)
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.ci_take(), np.concatenate([exp_a, exp_b]), "two calls")
    assert sk.ci_take().shape == (0,)
    # a take between two calls: the union is the whole, in order
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.ci_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    assert same(first, exp_a) and same(sk.ci_take(), exp_b)
    # begin twice: the second drops what is pending and takes the new gate, B, L and seed
    sk.compute_cgi(a_maps, a_frags, 1)
    gate = pc.oracle_gate(ref, b_maps, start)
    sk.ci_begin(**begin_args(7, 500, 9, gate))
    rc.reduce_check(ref, b_maps, start, 0, 10)
    exp_gated = expected(b, many_rows, b_cells.__getitem__, 7, 500, 9, gate)
    assert 0 < len(exp_gated) < len(many_rows)
    assert same(sk.ci_take(), exp_gated, "second begin")
    # the C call: ani_free releases the records, and n = 0 gives a NULL pointer
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_ci_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
    assert n.value == len(exp_gated) and rp.value
    raw = ctypes.string_at(rp.value, n.value * CI_DT.itemsize)
    lib.ani_free(rp)
    assert raw == exp_gated.tobytes()
    rp, n = ctypes.c_void_p(1), ctypes.c_size_t(5)
    chk(lib.ani_sketch_ci_take(sk.h, ctypes.byref(rp), ctypes.byref(n)))
    assert n.value == 0 and not rp.value
    # end: take and end are refused, mapping works and returns the same rows
    rc.reduce_check(ref, b_maps, start, 0, 10)               # pending records go with end
    sk.ci_end()
    expect_error(sk.ci_take, "take after end")
    expect_error(sk.ci_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.ci_begin(**arg)
    assert len(sk.ci_take()) == 0                            # nothing of before the end
    sk.ci_end()


def case_destroy_while_on(engine, frag_len=1000):
    """ani_sketch_destroy with the mode on and records pending releases them"""
    ref = rc.Ref(engine, frag_len)
    maps, frags = rc.list_random(ref.lay)
    ref.sk.ci_begin(**begin_args())
    ref.sk.compute_cgi(maps, frags, 0)
    ref.close()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    b = pc.bins_of(ref.lay)
    f32 = np.float32
    expect_error(sk.ci_take, "take without begin")
    expect_error(sk.ci_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.ci_begin(min_identity=v), "minIdentity " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.ci_begin(min_fragments=n), "minFragments %d" % n)
        expect_error(lambda: sk.ci_begin(replicates=n), "replicates %d" % n)
    for n in (1025, 2 ** 31 - 1):
        expect_error(lambda: sk.ci_begin(replicates=n), "replicates %d" % n)
    for level in (0.0, -5.0, 100.0, 99.96, 0.04, 1000.0, float("nan"), float("inf")):
        expect_error(lambda: sk.ci_begin(level=level), "level %r" % level)
    for permille in (0, -1, 1000, 2 ** 31 - 1, -2 ** 31):
        expect_error(lambda: chk(lib.ani_sketch_ci_begin(sk.h, 0.0, 1, 16, permille, 1)), "levelPermille %d" % permille)
    expect_error(sk.ci_take, "take after a refused begin")
    expect_error(lambda: chk(lib.ani_sketch_ci_begin(None, 0.0, 1, 16, 950, 1)), "begin(null)")
    rp, n = ctypes.c_void_p(), ctypes.c_size_t()
    expect_error(lambda: chk(lib.ani_sketch_ci_take(None, ctypes.byref(rp), ctypes.byref(n))), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_ci_end(None)), "end(null)")
    # a refused begin leaves a running mode, its gate, B, L and seed alone
    sk.ci_begin(**begin_args(7, 500, 3))
    rows = sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: sk.ci_begin(min_identity=101.0), "minIdentity 101")
    expect_error(lambda: sk.ci_begin(replicates=0), "replicates 0")
    expect_error(lambda: sk.ci_begin(replicates=1025), "replicates 1025")
    expect_error(lambda: sk.ci_begin(level=100.0), "level 100")
    expect_error(lambda: sk.ci_begin(min_fragments=0), "minFragments 0")
    expect_error(lambda: chk(lib.ani_sketch_ci_take(sk.h, None, ctypes.byref(n))), "take(sk, null)")
    expect_error(lambda: chk(lib.ani_sketch_ci_take(sk.h, ctypes.byref(rp), None)), "take(sk, rec, null)")
    cell = pc.cells(b, maps)
    assert same(sk.ci_take(), expected(b, rows, lambda qid: cell, 7, 500, 3), "after the refused begins")
    # the limits of the ranges are accepted
    sk.ci_begin(replicates=1, level=0.1, seed=0, min_identity=100.0, min_fragments=2 ** 31 - 1)
    sk.ci_begin(replicates=1024, level=99.9, seed=0xffffffff, min_identity=-0.0, min_fragments=1)
    sk.ci_end()


def case_together(ref):
    """the profile, the distributions, the hits and the intervals on at once: each equals its result alone, rows equal a run with
    everything off"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    p_gate, d_gate = pc.oracle_gate(ref, maps, start), (0.0, int(np.sort(rows["countSeq"])[len(rows) // 3]))
    h_gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 2)
    c_gate = (float(np.sort(rows["identity"])[len(rows) // 4]), 1)
    exp_c = expected(b, rows, cells_many(b, maps, start, 0).__getitem__, gate=c_gate)
    assert 0 < len(exp_c) < len(rows)
    # each alone
    sk.ci_begin(**begin_args(gate=c_gate))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    assert same(sk.ci_take(), exp_c, "alone")
    sk.ci_end()
    sk.hits_begin(*h_gate)
    rc.reduce_check(ref, maps, start, 0, 0)
    alone_h = sk.hits_take()
    sk.hits_end()
    sk.fragdist_begin(fc.DEFAULT_EDGES, *d_gate)
    rc.reduce_check(ref, maps, start, 0, 0)
    alone_d = sk.fragdist_take()
    sk.fragdist_end()
    sk.profile_begin(*p_gate)
    rc.reduce_check(ref, maps, start, 0, 0)
    alone_p = pc.read_raw(sk)
    sk.profile_end()
    assert len(alone_h) and len(alone_d[0])
    # all four
    sk.profile_begin(*p_gate)
    sk.fragdist_begin(fc.DEFAULT_EDGES, *d_gate)
    sk.hits_begin(*h_gate)
    sk.ci_begin(**begin_args(gate=c_gate))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    assert pc.read_raw(sk) == alone_p
    assert fc.same(sk.fragdist_take(), alone_d, "with the intervals on")
    assert hc.same(sk.hits_take(), alone_h, "with the intervals on")
    assert same(sk.ci_take(), exp_c, "with the three others on")
    sk.profile_end()
    sk.fragdist_end()
    sk.hits_end()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.ci_take(), exp_c, "after the others' end")
    sk.ci_end()


# ---- end to end: the mapper's own cells ----
E2E_GATE = pc.E2E_GATE


class EndToEnd(fc.EndToEnd):
    """the inputs, cells and rows of fragdist_cases.EndToEnd, and the intervals expected of them"""

    def __init__(self, engine):
        super().__init__(engine)
        self.ci_open = self.expect_ci(self.rows, (0.0, 1))
        self.ci_gated = self.expect_ci(self.rows, E2E_GATE)
        assert 0 < len(self.ci_gated) < len(self.ci_open) == len(self.rows)
        assert (self.ci_open["lowSum"] < self.ci_open["highSum"]).any()

    def expect_ci(self, rows, gate, ref_base=0, cells=None):
        return expected(self.b, rows, (cells or self.cells).__getitem__, gate=gate, ref_base=ref_base)

    def run(self, engine, config):
        sk = Sketch(engine, self.p, self.refs)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        sets = [engine.fragment_set(self.p, self.queries[:3]), engine.fragment_set(self.p, self.queries[3:])]
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 0), self.rows), config
        for gate, exp in ((E2E_GATE, self.ci_gated), ((0.0, 1), self.ci_open)):
            sk.ci_begin(**begin_args(gate=gate))
            assert rc.same_rows(sk.map_cgi_batch(self.queries, 0), self.rows), config
            assert same(sk.ci_take(), exp, config + ", map_cgi_batch, gate %r" % (gate,))
            assert rc.same_rows(sk.map_cgi_fragsets(sets, [0, 3]), self.rows), config
            assert same(sk.ci_take(), exp, config + ", map_cgi_fragsets, gate %r" % (gate,))
        for q in self.queries[:1]:
            sk.map_query(q)
            assert len(sk.ci_take()) == 0                  # ani_map_query adds nothing
        # a reference id base, and query ids that do not start at 0: the records carry the rows' ids
        sk.set_ref_id_base(500)
        moved = self.rows.copy()
        moved["refGenomeId"] += 500
        moved["qryGenomeId"] += 20
        exp = self.expect_ci(moved, E2E_GATE, 500, dict((q + 20, c) for q, c in self.cells.items()))
        sk.ci_begin(**begin_args(gate=E2E_GATE))
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 20), moved), config
        assert same(sk.ci_take(), exp, config + ", id base, map_cgi_batch")
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [20, 23]), moved), config
        assert same(sk.ci_take(), exp, config + ", id base, map_cgi_fragsets")
        for s in sets:
            s.close()
        sk.close()                                          # a sketch destroyed with the mode on releases its list


# ---- the command line: --ci ----
def fmt(x):
    return "%g" % float(x)


def ci_lines(out_lines, q_paths, r_paths, replicates, permille, seed, rec):
    """the .ci file for the lines of the -o file, from records whose query and reference ids are list positions"""
    at = dict(((int(r["qryGenomeId"]), int(r["refGenomeId"])), i) for i, r in enumerate(rec))
    qi, ri = dict((p, i) for i, p in enumerate(q_paths)), dict((p, i) for i, p in enumerate(r_paths))
    out = ["#replicates\t%d\tlevel\t%s\tseed\t%d" % (replicates, fmt(np.float32(permille / 10.0)), seed)]
    for line in out_lines:
        q, r, ani = line.split("\t")[:3]
        i = at.get((qi[q], ri[r]))
        if i is None:
            continue
        x = rec[i]
        out.append("\t".join([q, r, ani, fmt(x["low"]), fmt(x["high"]), str(int(x["count"]))]))
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
    plain, with_ci = os.path.join(tmp, "plain.out"), os.path.join(tmp, "ci.out")
    p = engine.params(pc.E2E_K, pc.E2E_FRAG_LEN)

    # the restatement over each query's own mappings against one sketch of all references (ids = list positions)
    sk = Sketch(engine, p, refs)
    b = pc.Bins([len(c) for g in refs for c in g], [g for g, cs in enumerate(refs) for _ in cs], pc.E2E_FRAG_LEN)
    cells, rows = {}, []
    for qi, q in enumerate(queries):
        maps, total = sk.map_query(q)
        cells[qi] = pc.cells(b, maps)
        rows.append(sk.compute_cgi(maps, total, qi))
    sk.close()
    rows = np.concatenate(rows)

    def run(out, opts):
        r = subprocess.run(base + ["-o", out] + opts, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]

    run(plain, [])
    # the defaults: a line for every -o line; every other file is what it was
    run(with_ci, ["--ci"])
    produced = sorted(f[len("plain.out"):] for f in os.listdir(tmp) if f.startswith("plain.out"))
    assert produced == ["", ".matrix"] and sorted(f[len("ci.out"):] for f in os.listdir(tmp) if f.startswith("ci.out")) == ["", ".ci", ".matrix"]
    for suffix in produced:
        assert open(plain + suffix, "rb").read() == open(with_ci + suffix, "rb").read(), suffix
    out_lines = open(plain).read().splitlines()
    assert len(out_lines) >= 6
    got = open(with_ci + ".ci").read().splitlines()
    exp = ci_lines(out_lines, q_paths, r_paths, 200, 950, 1, expected(b, rows, cells.__getitem__, 200, 950, 1))
    assert got == exp, "%s: %d lines, expected %d; first difference %r" % (mode, len(got), len(exp), next(((x, y) for x, y in zip(got, exp) if x != y), None))
    assert len(got) == len(out_lines) + 1 and got[0] == "#replicates\t200\tlevel\t95\tseed\t1"
    if mode == "lists":
        # lines of -o that --minFraction drops have no line here: the records are joined on (query, reference)
        strict, strict_ci = os.path.join(tmp, "strict.out"), os.path.join(tmp, "strict_ci.out")
        run(strict, ["--minFraction", "0.9"])
        run(strict_ci, ["--minFraction", "0.9", "--ci"])
        strict_lines = open(strict).read().splitlines()
        assert 0 < len(strict_lines) < len(out_lines) and open(strict_ci).read().splitlines() == strict_lines
        assert open(strict_ci + ".ci").read().splitlines() == ci_lines(strict_lines, q_paths, r_paths, 200, 950, 1, expected(b, rows, cells.__getitem__, 200, 950, 1))
    # a gate that drops the record of at least one -o line and keeps at least one; B, level and seed of the caller's
    ids = sorted(set(float(line.split("\t")[2]) for line in out_lines))
    assert ids[-1] - ids[0] > 0.01
    gate = (float("%.4f" % ((ids[0] + ids[-1]) / 2)), 2)
    opts = ["--ci", "--ciReplicates", "33", "--ciLevel", "99.5", "--ciSeed", "4000000000", "--ciMinANI", str(gate[0]), "--ciMinFragments", str(gate[1])]
    run(with_ci, opts)
    for suffix in produced:
        assert open(plain + suffix, "rb").read() == open(with_ci + suffix, "rb").read(), suffix
    got = open(with_ci + ".ci").read().splitlines()
    assert got == ci_lines(out_lines, q_paths, r_paths, 33, 995, 4000000000, expected(b, rows, cells.__getitem__, 33, 995, 4000000000, gate)), mode
    assert got[0] == "#replicates\t33\tlevel\t99.5\tseed\t4000000000" and 1 < len(got) < len(out_lines) + 1, (len(got), len(out_lines))
    if mode == "lists":
        # with the other per-pair files beside it
        both = os.path.join(tmp, "both.out")
        run(both, opts + ["--profile", "--fragDist", "--hits"])
        assert open(both + ".ci").read().splitlines() == got
        assert open(both, "rb").read() == open(plain, "rb").read() and all(os.path.exists(both + s) for s in (".profile", ".fragdist", ".hits"))
        # the five sub-options are refused by name without --ci, and bad values before anything is mapped
        for opts, msg in ((["--ciReplicates", "100"], b"--ciReplicates needs --ci"), (["--ciLevel", "90"], b"--ciLevel needs --ci"),
                          (["--ciSeed", "5"], b"--ciSeed needs --ci"), (["--ciMinANI", "90"], b"--ciMinANI needs --ci"),
                          (["--ciMinFragments", "5"], b"--ciMinFragments needs --ci"),
                          (["--ci", "--ciReplicates", "0"], b"--ciReplicates takes"), (["--ci", "--ciReplicates", "1025"], b"--ciReplicates takes"),
                          (["--ci", "--ciLevel", "0"], b"--ciLevel takes"), (["--ci", "--ciLevel", "100"], b"--ciLevel takes"),
                          (["--ci", "--ciLevel", "95.05"], b"--ciLevel takes"), (["--ci", "--ciLevel", "nan"], b"--ciLevel takes"),
                          (["--ci", "--ciLevel", "95x"], b"--ciLevel takes"), (["--ci", "--ciSeed", "-1"], b"--ciSeed takes"),
                          (["--ci", "--ciSeed", "4294967296"], b"--ciSeed takes"),
                          (["--ci", "--ciMinANI", "-1"], b"--ciMinANI takes"), (["--ci", "--ciMinANI", "100.5"], b"--ciMinANI takes"),
                          (["--ci", "--ciMinFragments", "0"], b"--ciMinFragments takes")):
            r = subprocess.run(base + ["-o", os.path.join(tmp, "refused.out")] + opts, capture_output=True)
            assert r.returncode == 1 and msg in r.stderr, (opts, r.stderr[-500:])
        assert not os.path.exists(os.path.join(tmp, "refused.out"))
