"""Cases for the bootstrap replicate records (kernels/boot.hpp: k_boot_records behind the intervals' k_ci_flags and k_ci_list; boot_stage,
collect_rows and ani_sketch_boot_begin / _take / _end in engine_map.hip), shared by the GPU tests (-m gpu, product library) and the
CPU-emulation tests (not gpu, tests/emu build): test_boot.py.

The reference is a numpy restatement of rule 1 of the boot records in include/ani_abi.h from the pieces of ci_cases.py (draws, fix)
over the cells of profile_cases.py: per row that passes the gate, the genome's non-empty cells in bin order, fix of each, the draws of
the stated hash and the replicate sums in replicate order.  The ids and the order of the expected records are those of the rows the
same call returned.  Every comparison is on bits; there is no tolerance.

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins) and the engines are those of reduce_cases.py
and fragdist_cases.py."""
import ctypes

import numpy as np

import ci_cases as cc
import fragdist_cases as fc
import profile_cases as pc
import reduce_cases as rc
from fastani_amd.api import BOOT_DT, Sketch, boot_identity

LISTS = fc.LISTS
LISTS_ONE = fc.LISTS_ONE
assert all(x in LISTS_ONE for x in ("all_equal", "n1", "low_bits"))
LISTS_MANY = fc.LISTS_MANY
LISTS_GATE = fc.LISTS_GATE
B_ONE = cc.B_ONE                                        # replicates of the engine tests outside the sweep, as ci_cases
SWEEP_B = (1, 2, 7, 63, 64, 65, 255, 256, 257, 1024)    # every stride border of a workgroup of 256 and of a wave of 64, on both builds
bits = pc.bits
expect_error = pc.expect_error
cells_many = fc.cells_many


# ---- rule 1 ----
def replicate_sums(f, replicates, seed):
    """F in bin order -> (sum, S[0 .. B)): the definition, no shortcut"""
    f = np.asarray(f, dtype=np.uint64)
    return int(f.sum(dtype=np.uint64)), f[cc.draws(len(f), replicates, seed)].sum(axis=1, dtype=np.uint64)


def expected(b, rows, cell_of, replicates=B_ONE, seed=1, gate=(0.0, 1), ref_base=0):
    """(records, sums) of the pairs of `rows` (the rows a call returned, in its order) that pass the gate; cell_of(qryGenomeId) = that
    query's cells (profile_cases.cells); a row's genome is refGenomeId - ref_base"""
    min_bits, min_frag = pc.gate_bits(gate[0]), int(gate[1])
    rec, sums = [], []
    for row in rows:
        if int(row["countSeq"]) < min_frag or int(bits(row["identity"])) < min_bits:
            continue
        g = int(row["refGenomeId"]) - ref_base
        cell = cell_of(int(row["qryGenomeId"]))[int(b.genome_start[g]):int(b.genome_start[g + 1])]
        v = cell[cell != 0]                                 # bin order
        assert len(v) == int(row["countSeq"])               # rule 1
        total, s = replicate_sums(cc.fix(v), replicates, seed)
        r = np.zeros(1, dtype=BOOT_DT)
        r["refGenomeId"], r["qryGenomeId"], r["count"], r["replicates"], r["sum"] = row["refGenomeId"], row["qryGenomeId"], len(v), replicates, total
        rec.append(r)
        sums.append(s)
    if not rec:
        return np.zeros(0, dtype=BOOT_DT), np.zeros((0, replicates), dtype=np.uint64)
    return np.concatenate(rec), np.stack(sums)


def same(got, exp, what=""):
    (grec, gsum), (erec, esum) = got, exp
    assert grec.dtype == BOOT_DT and gsum.dtype == np.uint64, (grec.dtype, gsum.dtype)
    assert grec.shape == erec.shape and gsum.shape == esum.shape, (what, grec.shape, erec.shape, gsum.shape, esum.shape)
    if grec.tobytes() != erec.tobytes():
        bad = [i for i in range(len(grec)) if grec[i].tobytes() != erec[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, the first at %d:\n%r\n%r" % (what, len(bad), len(grec), bad[0], grec[bad[0]], erec[bad[0]]))
    if gsum.tobytes() != esum.tobytes():
        bad = np.argwhere(gsum != esum)
        raise AssertionError("%s: %d of %d sums differ, the first at %r: %d, expected %d" % (what, len(bad), gsum.size, tuple(bad[0]), gsum[tuple(bad[0])], esum[tuple(bad[0])]))
    return True


def begin_args(replicates=B_ONE, seed=1, gate=(0.0, 1)):
    return dict(replicates=replicates, seed=seed, min_identity=gate[0], min_fragments=gate[1])


def run_one(sk, maps, frags, qid, **kw):
    sk.boot_begin(**kw)
    rows = sk.compute_cgi(maps, frags, qid)
    got = sk.boot_take()
    sk.boot_end()
    return rows, got


# ---- the restatement on its own: CPU only, no engine ----
def case_restatement(name):
    """the restatement against the intervals' (itself held to the oracle and to statistics in test_ci.py): rule 2 on the CPU, the bounds of a
    sum, and the constant pairs"""
    lay = rc.Layout(1000)
    b = pc.bins_of(lay)
    maps, frags = LISTS[name](lay)
    rows = pc.rows_of(b, pc.cells(b, maps), frags, 0)
    cell = pc.cells(b, maps)
    for replicates, permille, seed in ((B_ONE, 950, 1), (200, 950, 7), (7, 500, 0)):
        rec, sums = expected(b, rows, lambda qid: cell, replicates, seed)
        ci = cc.expected(b, rows, lambda qid: cell, replicates, permille, seed)
        assert len(rec) == len(rows) == len(ci) and sums.shape == (len(rec), replicates)
        lo, hi = cc.ranks(replicates, permille)
        s = np.sort(sums, axis=1)
        assert np.array_equal(s[:, lo], ci["lowSum"]) and np.array_equal(s[:, hi], ci["highSum"]) and np.array_equal(rec["sum"], ci["sum"])
        for r, x, row in zip(rec, sums, rows):
            g = int(row["refGenomeId"])
            v = cell[int(b.genome_start[g]):int(b.genome_start[g + 1])]
            f = cc.fix(v[v != 0])
            assert int(f.min()) * len(f) <= int(x.min()) and int(x.max()) <= int(f.max()) * len(f)
            if int(f.min()) == int(f.max()):
                assert (x == r["sum"]).all()
    if name in ("all_equal", "n1"):
        assert (sums == rec["sum"][:, None]).all()
    if name == "n1":
        assert len(rec) == 1 and int(rec["count"][0]) == 1


def case_identity():
    """boot_identity is rule 3, bit for bit, at the borders of float rounding"""
    rec = np.zeros(4, dtype=BOOT_DT)
    rec["count"] = (1, 3, 1678, 2560)
    sums = np.array([[104857600, 1], [299999999, 300000001], [175000000000, 175953412096], [2560 * 104857600, 2560 * 104857599]], dtype=np.uint64)
    got = boot_identity(rec, sums)
    assert got.dtype == np.float32 and got.shape == (4, 2)
    for i in range(4):
        for r in range(2):
            assert bits(got[i, r]) == bits(np.float32(np.float64(int(sums[i, r])) / (np.float64(int(rec["count"][i])) * 1048576.0)))
    assert got[0, 0] == np.float32(100.0) and got[3, 0] == np.float32(100.0)


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
            rec, sums = exp
            assert len(rec) == len(exp_rows)
            if name == "dense":
                assert sorted(int(c) for c in rec["count"]) == [65, 129] and (sums.min(axis=1) < sums.max(axis=1)).all()
            if name == "n1":
                assert len(rec) == 1 and int(rec["count"][0]) == 1 and (sums == rec["sum"][0]).all()
            if name == "n0":
                assert len(rec) == 0
            if name == "all_equal":
                assert (sums == rec["sum"][:, None]).all()


def case_sweep(ref, replicates):
    """`dense` (129 and 65 cells) and `random` at `replicates`"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    for name in ("dense", "random"):
        maps, frags = LISTS[name](lay)
        rows = ref.expected(maps, frags, 0)
        cell = pc.cells(b, maps)
        exp = expected(b, rows, lambda qid: cell, replicates, 3)
        got_rows, got = run_one(sk, maps, frags, 0, **begin_args(replicates, 3))
        assert rc.same_rows(got_rows, rows) and same(got, exp, "%s, B %d" % (name, replicates))
        assert got[1].shape == (len(rows), replicates) and (got[0]["replicates"] == replicates).all()


# ---- several queries in one table: ani_reduce_check ----
def case_many(ref, name, gated=False, also=None):
    """`also`: a second Ref (the default engine's) whose records must equal this one's"""
    lay = ref.lay
    b = pc.bins_of(lay)
    maps0, frags = LISTS[name](lay)
    for maps, start, genome_base in cc.many_runs(maps0, frags, gated):
        gate = pc.oracle_gate(ref, maps, start) if gated else (0.0, 1)
        exp_rows = rc.expected_many(ref, maps, start, 7)
        exp = expected(b, exp_rows, cells_many(b, maps, start, 7).__getitem__, gate=gate)
        assert (0 < len(exp[0]) < len(exp_rows)) if gated else len(exp[0]) == len(exp_rows)
        for order in (rc.in_order, rc.shuffled):
            what = "%s, fragLen %d, queries %r, genomeBase %d, gate %r, %s" % (name, lay.frag_len, start, genome_base, gate, order.__name__)
            for r in (ref,) if also is None else (ref, also):
                r.sk.boot_begin(**begin_args(gate=gate))
                got_rows = rc.reduce_check(r, order(maps), start, genome_base, 7)
                got = r.sk.boot_take()
                r.sk.boot_end()
                assert rc.same_rows(got_rows, exp_rows), what
                assert same(got, exp, what)


def case_gate_edges(ref):
    """the gate's own edges on `random` over 5 queries, as ci_cases.case_gate_edges"""
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
        sk.boot_begin(**begin_args(gate=gate))
        got_rows = rc.reduce_check(ref, maps, start, 0, 0)
        got = sk.boot_take()
        sk.boot_end()
        assert rc.same_rows(got_rows, rows), gate
        assert len(got[0]) == n, (gate, len(got[0]), n)
        assert same(got, expected(b, rows, cm.__getitem__, gate=gate), repr(gate))


def case_seeds(ref):
    """seeds 0, 1, 2 and 2^32 - 1: each equals the restatement, two seeds differ, the same seed twice gives equal records"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_random(lay)
    rows = ref.expected(maps, frags, 0)
    cell = pc.cells(b, maps)
    got = {}
    for seed in (1, 2, 1, 0, 0xffffffff):
        _, x = run_one(sk, maps, frags, 0, **begin_args(seed=seed))
        assert same(x, expected(b, rows, lambda qid: cell, seed=seed), "seed %d" % seed)
        if seed in got:
            assert x[1].tobytes() == got[seed][1].tobytes()
        got[seed] = x
    assert (got[1][1] != got[2][1]).any() and np.array_equal(got[1][0]["sum"], got[2][0]["sum"])


# ---- rule 2: the intervals beside the replicate records, in one call ----
def case_intervals(ref):
    """the intervals on at the same seed and B: sorted sums at lowRank / highRank are lowSum / highSum, sum is sum; the intervals at another
    seed and B change nothing here, and these records change nothing there"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    cm = cells_many(b, maps, start, 0)
    replicates, permille, seed = B_ONE, 900, 5
    exp = expected(b, rows, cm.__getitem__, replicates, seed)
    sk.ci_begin(**cc.begin_args(replicates, permille, seed))
    sk.boot_begin(**begin_args(replicates, seed))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    ci, got = sk.ci_take(), sk.boot_take()
    assert same(got, exp, "with the intervals on") and cc.same(ci, cc.expected(b, rows, cm.__getitem__, replicates, permille, seed))
    lo, hi = cc.ranks(replicates, permille)
    s = np.sort(got[1], axis=1)
    assert len(ci) == len(got[0]) and np.array_equal(ci["refGenomeId"], got[0]["refGenomeId"]) and np.array_equal(ci["qryGenomeId"], got[0]["qryGenomeId"])
    assert np.array_equal(s[:, lo], ci["lowSum"]) and np.array_equal(s[:, hi], ci["highSum"]) and np.array_equal(got[0]["sum"], ci["sum"])
    assert (ci["lowSum"] < ci["highSum"]).any()
    # the intervals at another seed, B and gate: two modes that do not see each other
    gate = (float(np.sort(rows["identity"])[len(rows) // 3]), 1)
    sk.ci_begin(**cc.begin_args(7, 500, 9, gate))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    ci2, got2 = sk.ci_take(), sk.boot_take()
    assert same(got2, exp, "the intervals at another seed") and cc.same(ci2, cc.expected(b, rows, cm.__getitem__, 7, 500, 9, gate))
    assert 0 < len(ci2) < len(rows)
    sk.ci_end()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.boot_take(), exp, "after the intervals' end")
    sk.boot_end()


# ---- life cycle and arguments ----
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

    off_a, off_b = sk.compute_cgi(a_maps, a_frags, 1), rc.reduce_check(ref, b_maps, start, 0, 10)
    assert rc.same_rows(off_a, a_rows) and rc.same_rows(off_b, many_rows)
    # two calls, one take: call order; the second take is empty
    sk.boot_begin(**arg)
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    assert same(sk.boot_take(), (np.concatenate([exp_a[0], exp_b[0]]), np.concatenate([exp_a[1], exp_b[1]])), "two calls")
    rec, sums = sk.boot_take()
    assert rec.shape == (0,) and sums.shape == (0, B_ONE)
    # a take between two calls: the union is the whole, in order
    sk.compute_cgi(a_maps, a_frags, 1)
    first = sk.boot_take()
    rc.reduce_check(ref, b_maps, start, 0, 10)
    assert same(first, exp_a) and same(sk.boot_take(), exp_b)
    # begin twice: the second drops what is pending and takes the new gate, B and seed
    sk.compute_cgi(a_maps, a_frags, 1)
    gate = pc.oracle_gate(ref, b_maps, start)
    sk.boot_begin(**begin_args(7, 9, gate))
    rc.reduce_check(ref, b_maps, start, 0, 10)
    exp_gated = expected(b, many_rows, b_cells.__getitem__, 7, 9, gate)
    assert 0 < len(exp_gated[0]) < len(many_rows)
    assert same(sk.boot_take(), exp_gated, "second begin")
    # the C call: ani_free releases both buffers, n = 0 gives NULL pointers, and sums may be null
    lib, chk = ref.engine.lib, ref.engine._chk
    rc.reduce_check(ref, b_maps, start, 0, 10)
    rp, sp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    chk(lib.ani_sketch_boot_take(sk.h, ctypes.byref(rp), ctypes.byref(sp), ctypes.byref(n)))
    assert n.value == len(exp_gated[0]) and rp.value and sp.value
    raw, raw_sums = ctypes.string_at(rp.value, n.value * BOOT_DT.itemsize), ctypes.string_at(sp.value, n.value * 7 * 8)
    lib.ani_free(rp)
    lib.ani_free(sp)
    assert raw == exp_gated[0].tobytes() and raw_sums == exp_gated[1].tobytes()
    rp, sp, n = ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_size_t(5)
    chk(lib.ani_sketch_boot_take(sk.h, ctypes.byref(rp), ctypes.byref(sp), ctypes.byref(n)))
    assert n.value == 0 and not rp.value and not sp.value
    rc.reduce_check(ref, b_maps, start, 0, 10)
    chk(lib.ani_sketch_boot_take(sk.h, ctypes.byref(rp), None, ctypes.byref(n)))
    assert n.value == len(exp_gated[0]) and ctypes.string_at(rp.value, n.value * BOOT_DT.itemsize) == exp_gated[0].tobytes()
    lib.ani_free(rp)
    # end: take and end are refused, mapping works and returns the same rows
    rc.reduce_check(ref, b_maps, start, 0, 10)               # pending records go with end
    sk.boot_end()
    expect_error(sk.boot_take, "take after end")
    expect_error(sk.boot_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), off_a) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 10), off_b)
    sk.boot_begin(**arg)
    assert len(sk.boot_take()[0]) == 0                       # nothing of before the end
    sk.boot_end()


def case_destroy_while_on(engine, frag_len=1000):
    """ani_sketch_destroy with the mode on and records pending releases them"""
    ref = rc.Ref(engine, frag_len)
    maps, frags = rc.list_random(ref.lay)
    ref.sk.boot_begin(**begin_args())
    ref.sk.compute_cgi(maps, frags, 0)
    ref.close()


def case_arguments(ref):
    sk, lib, chk = ref.sk, ref.engine.lib, ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    b = pc.bins_of(ref.lay)
    f32 = np.float32
    expect_error(sk.boot_take, "take without begin")
    expect_error(sk.boot_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.boot_begin(min_identity=v), "minIdentity " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.boot_begin(min_fragments=n), "minFragments %d" % n)
        expect_error(lambda: sk.boot_begin(replicates=n), "replicates %d" % n)
    for n in (1025, 2 ** 31 - 1):
        expect_error(lambda: sk.boot_begin(replicates=n), "replicates %d" % n)
    expect_error(sk.boot_take, "take after a refused begin")
    expect_error(lambda: chk(lib.ani_sketch_boot_begin(None, 0.0, 1, 16, 1)), "begin(null)")
    rp, sp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    expect_error(lambda: chk(lib.ani_sketch_boot_take(None, ctypes.byref(rp), ctypes.byref(sp), ctypes.byref(n))), "take(null)")
    expect_error(lambda: chk(lib.ani_sketch_boot_end(None)), "end(null)")
    # a refused begin leaves a running mode, its gate, B and seed alone
    sk.boot_begin(**begin_args(7, 3))
    rows = sk.compute_cgi(maps, frags, 0)
    expect_error(lambda: sk.boot_begin(min_identity=101.0), "minIdentity 101")
    expect_error(lambda: sk.boot_begin(replicates=0), "replicates 0")
    expect_error(lambda: sk.boot_begin(replicates=1025), "replicates 1025")
    expect_error(lambda: sk.boot_begin(min_fragments=0), "minFragments 0")
    expect_error(lambda: chk(lib.ani_sketch_boot_take(sk.h, None, ctypes.byref(sp), ctypes.byref(n))), "take(sk, null)")
    expect_error(lambda: chk(lib.ani_sketch_boot_take(sk.h, ctypes.byref(rp), ctypes.byref(sp), None)), "take(sk, rec, sums, null)")
    cell = pc.cells(b, maps)
    assert same(sk.boot_take(), expected(b, rows, lambda qid: cell, 7, 3), "after the refused begins")
    # the limits of the ranges are accepted
    sk.boot_begin(replicates=1, seed=0, min_identity=100.0, min_fragments=2 ** 31 - 1)
    sk.boot_begin(replicates=1024, seed=0xffffffff, min_identity=-0.0, min_fragments=1)
    sk.boot_end()


def case_together(ref):
    """the profile, the distributions, the hits, the intervals, paint and synteny on beside the replicate records: each equals its result
    alone, rows equal a run with everything off"""
    lay, sk = ref.lay, ref.sk
    b = pc.bins_of(lay)
    maps, frags = rc.list_ties(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    p_gate, d_gate = pc.oracle_gate(ref, maps, start), (0.0, int(np.sort(rows["countSeq"])[len(rows) // 3]))
    h_gate = (float(np.sort(rows["identity"])[len(rows) // 2]), 2)
    c_gate = (float(np.sort(rows["identity"])[len(rows) // 4]), 1)
    b_gate = (float(np.sort(rows["identity"])[len(rows) // 5]), 2)
    exp = expected(b, rows, cells_many(b, maps, start, 0).__getitem__, gate=b_gate)
    assert 0 < len(exp[0]) < len(rows)
    # each alone
    sk.boot_begin(**begin_args(gate=b_gate))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    assert same(sk.boot_take(), exp, "alone")
    sk.boot_end()
    alone = {}
    modes = (("ci", lambda: sk.ci_begin(**cc.begin_args(gate=c_gate)), sk.ci_take, sk.ci_end),
             ("hits", lambda: sk.hits_begin(*h_gate), sk.hits_take, sk.hits_end),
             ("fragdist", lambda: sk.fragdist_begin(fc.DEFAULT_EDGES, *d_gate), sk.fragdist_take, sk.fragdist_end),
             ("profile", lambda: sk.profile_begin(*p_gate), lambda: pc.read_raw(sk), sk.profile_end),
             ("paint", sk.paint_begin, sk.paint_take, sk.paint_end),
             ("synteny", lambda: sk.synteny_begin(*h_gate), sk.synteny_take, sk.synteny_end))
    for name, begin, take, end in modes:
        begin()
        rc.reduce_check(ref, maps, start, 0, 0)
        alone[name] = take()
        end()
    assert len(alone["ci"]) and len(alone["hits"]) and len(alone["fragdist"][0]) and len(alone["paint"]) and len(alone["synteny"][0])
    # all seven
    for name, begin, take, end in modes:
        begin()
    sk.boot_begin(**begin_args(gate=b_gate))
    assert rc.same_rows(rc.reduce_check(ref, maps, start, 0, 0), rows)
    for name, begin, take, end in modes:
        got = take()
        if name == "profile":
            assert got == alone[name]
        elif name in ("fragdist", "synteny"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, alone[name])), name
        else:
            assert got.tobytes() == alone[name].tobytes(), name
    assert same(sk.boot_take(), exp, "with the six others on")
    for name, begin, take, end in modes:
        end()
    rc.reduce_check(ref, maps, start, 0, 0)
    assert same(sk.boot_take(), exp, "after the others' end")
    sk.boot_end()


# ---- end to end: the mapper's own cells ----
E2E_GATE = pc.E2E_GATE


class EndToEnd(fc.EndToEnd):
    """the inputs, cells and rows of fragdist_cases.EndToEnd, and the replicate records expected of them"""

    def __init__(self, engine):
        super().__init__(engine)
        self.boot_open = self.expect_boot(self.rows, (0.0, 1))
        self.boot_gated = self.expect_boot(self.rows, E2E_GATE)
        assert 0 < len(self.boot_gated[0]) < len(self.boot_open[0]) == len(self.rows)
        assert (self.boot_open[1].min(axis=1) < self.boot_open[1].max(axis=1)).any()

    def expect_boot(self, rows, gate, ref_base=0, cells=None):
        return expected(self.b, rows, (cells or self.cells).__getitem__, gate=gate, ref_base=ref_base)

    def run(self, engine, config):
        sk = Sketch(engine, self.p, self.refs)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        sets = [engine.fragment_set(self.p, self.queries[:3]), engine.fragment_set(self.p, self.queries[3:])]
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 0), self.rows), config
        for gate, exp in ((E2E_GATE, self.boot_gated), ((0.0, 1), self.boot_open)):
            sk.boot_begin(**begin_args(gate=gate))
            assert rc.same_rows(sk.map_cgi_batch(self.queries, 0), self.rows), config
            assert same(sk.boot_take(), exp, config + ", map_cgi_batch, gate %r" % (gate,))
            assert rc.same_rows(sk.map_cgi_fragsets(sets, [0, 3]), self.rows), config
            assert same(sk.boot_take(), exp, config + ", map_cgi_fragsets, gate %r" % (gate,))
        for q in self.queries[:1]:
            sk.map_query(q)
            assert len(sk.boot_take()[0]) == 0             # ani_map_query adds nothing
        # a reference id base, and query ids that do not start at 0: the records carry the rows' ids
        sk.set_ref_id_base(500)
        moved = self.rows.copy()
        moved["refGenomeId"] += 500
        moved["qryGenomeId"] += 20
        exp = self.expect_boot(moved, E2E_GATE, 500, dict((q + 20, c) for q, c in self.cells.items()))
        sk.boot_begin(**begin_args(gate=E2E_GATE))
        assert rc.same_rows(sk.map_cgi_batch(self.queries, 20), moved), config
        assert same(sk.boot_take(), exp, config + ", id base, map_cgi_batch")
        assert rc.same_rows(sk.map_cgi_fragsets(sets, [20, 23]), moved), config
        assert same(sk.boot_take(), exp, config + ", id base, map_cgi_fragsets")
        for s in sets:
            s.close()
        sk.close()                                          # a sketch destroyed with the mode on releases its lists
