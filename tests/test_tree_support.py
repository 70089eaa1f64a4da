"""Clade support of a tree over replicate trees (ani_tree_support, a host function) against a plain-Python restatement on frozensets of
leaves, and the composed call ani_tree_support_bootstrap (Engine.tree_support_bootstrap) against the composition it is defined as:
the method's tree per replicate through Engine.tree_average / tree_nj / tree_single, then tree_support.  CPU: the tests/emu build of
the library; GPU (-m gpu): the product library.  Everything is compared exactly."""
import ctypes

import numpy as np
import pytest

import boot_cases as bc
import ci_cases as cc
from fastani_amd.api import BOOT_DT, AniError, boot_identity, tree_support
from test_cluster import make_rows
from test_tree import expected as upgma

ERR_ARG, ERR_LIMIT = -1, -4


# ---- the restatement ----
def leaf_sets(children, n):
    """rule 1: the leaf set of every node, leaves first"""
    sets = [frozenset([i]) for i in range(n)]
    for a, b in np.asarray(children).reshape(-1, 2).tolist():
        sets.append(sets[a] | sets[b])
    return sets


def restated(children, reps, unrooted=False):
    children = np.asarray(children).reshape(-1, 2)
    n = len(children) + 1
    main, everything = leaf_sets(children, n), frozenset(range(n))
    have = [set(leaf_sets(r, n)) for r in reps]
    out = []
    for s in range(n - 1):
        v = main[n + s]
        if unrooted and len(v) >= n - 1:
            out.append(len(reps))
        else:
            out.append(sum(1 for h in have if v in h or (unrooted and (everything - v) in h)))
    return np.array(out, dtype=np.uint32)


def check(lib, children, reps, unrooted=False, want=None):
    children = np.asarray(children, dtype=np.int32).reshape(-1, 2)
    reps = np.asarray(reps, dtype=np.int32).reshape(-1, len(children), 2)
    got = tree_support(children, reps, unrooted, lib=lib)
    exp = restated(children, reps, unrooted)
    assert got.dtype == np.uint32 and got.tolist() == exp.tolist(), (children.tolist(), reps.tolist(), unrooted, got.tolist(), exp.tolist())
    if want is not None:
        assert got.tolist() == list(want), (got.tolist(), want)
    return got


# ---- trees ----
def caterpillar(order):
    """((((o0, o1), o2), o3), ...)"""
    n = len(order)
    ch = np.empty((n - 1, 2), dtype=np.int32)
    ch[0] = (order[0], order[1])
    for s in range(1, n - 1):
        ch[s] = (n + s - 1, order[s + 1])
    return ch


def split_tree(order, rng):
    """a random tree whose clades are runs of `order`: recursive bipartition, the records in post-order"""
    n, rec = len(order), []

    def build(lo, hi):
        if hi - lo == 1:
            return int(order[lo])
        cut = int(rng.integers(lo + 1, hi))
        a, b = build(lo, cut), build(cut, hi)
        rec.append((a, b))
        return n + len(rec) - 1

    build(0, n)
    return np.array(rec, dtype=np.int32).reshape(n - 1, 2)


def rewritten(children, rng):
    """the same rooted tree: children swapped at random, the records in another order that still names a node after its record"""
    children = np.asarray(children).reshape(-1, 2)
    n = len(children) + 1
    new_id, done, out = dict((i, i) for i in range(n)), set(), []
    while len(out) < n - 1:
        ready = [s for s in range(n - 1) if s not in done and all(int(c) in new_id for c in children[s])]
        s = ready[int(rng.integers(len(ready)))]
        a, b = (new_id[int(c)] for c in children[s])
        out.append((b, a) if rng.integers(2) else (a, b))
        new_id[n + s] = n + len(out) - 1
        done.add(s)
    return np.array(out, dtype=np.int32)


# ---- ani_tree_support: hand-written trees ----
def hand_written(lib):
    # n = 1 (and 0): nothing read or written
    assert lib.ani_tree_support(None, 1, None, 3, 0, None) == 0 and lib.ani_tree_support(None, 0, None, 0, 1, None) == 0
    # n = 2: one record, all leaves
    check(lib, [(0, 1)], [[(0, 1)], [(1, 0)]], False, [2])
    check(lib, [(0, 1)], [[(0, 1)], [(1, 0)]], True, [2])
    check(lib, [(0, 1)], np.zeros((0, 1, 2)), False, [0])
    # n = 3: ((0,1),2) against itself, ((0,2),1) and ((1,2),0)
    reps3 = [[(0, 1), (3, 2)], [(0, 2), (3, 1)], [(1, 2), (0, 3)]]
    check(lib, [(0, 1), (3, 2)], reps3, False, [1, 3])
    check(lib, [(0, 1), (3, 2)], reps3, True, [3, 3])       # three leaves: every split is trivial
    # n = 4: ((0,1),(2,3))
    main4 = [(0, 1), (2, 3), (4, 5)]
    reps4 = [[(2, 3), (0, 1), (5, 4)], [(0, 1), (4, 2), (5, 3)], [(0, 2), (1, 3), (4, 5)], [(1, 0), (2, 4), (3, 5)]]
    check(lib, main4, reps4, False, [3, 1, 4])
    check(lib, main4, reps4, True, [3, 3, 4])               # {2,3} is the other side of {0,1}
    # n = 5: (((0,1),2),(3,4))
    main5 = [(0, 1), (5, 2), (3, 4), (6, 7)]
    reps5 = [main5, [(3, 4), (0, 1), (2, 6), (5, 7)], [(1, 2), (0, 5), (3, 4), (6, 7)], [(0, 1), (5, 3), (6, 2), (7, 4)], [(0, 3), (1, 4), (5, 6), (7, 2)]]
    check(lib, main5, reps5, False, [3, 3, 3, 5])
    check(lib, main5, reps5, True, [3, 3, 3, 5])


def same_tree_rewritten(lib):
    rng = np.random.default_rng(5)
    for n in (2, 3, 7, 33):
        main = split_tree(rng.permutation(n), rng)
        reps = [rewritten(main, rng) for _ in range(4)]
        for unrooted in (False, True):
            check(lib, main, reps, unrooted, [4] * (n - 1))


def caterpillar_and_balanced(lib):
    n = 16
    cat = caterpillar(np.arange(n))
    rec, level = [], list(range(n))
    while len(level) > 1:                                   # the balanced tree over the same order
        nxt = []
        for i in range(0, len(level), 2):
            rec.append((level[i], level[i + 1]))
            nxt.append(n + len(rec) - 1)
        level = nxt
    bal = np.array(rec, dtype=np.int32)
    # the caterpillar's clades {0..k}: the balanced tree has those with k + 1 a power of two
    check(lib, cat, [bal], False, [1 if (k + 2) & (k + 1) == 0 else 0 for k in range(n - 1)])
    got = check(lib, bal, [cat, bal], False)
    assert got.tolist() == [2 if leaf_sets(bal, n)[n + s] in set(leaf_sets(cat, n)) else 1 for s in range(n - 1)]
    check(lib, cat, [bal, cat], True)


def one_clade_moved(lib):
    # ((0,1),(2,3)),((4,5),6) and the same tree with leaf 6 moved next to (0,1)
    main = [(0, 1), (2, 3), (7, 8), (4, 5), (10, 6), (9, 11)]
    moved = [(0, 1), (7, 6), (2, 3), (8, 9), (4, 5), (10, 11)]
    check(lib, main, [main, moved], False, [2, 2, 1, 2, 1, 2])
    check(lib, main, [main, moved], True, [2, 2, 1, 2, 1, 2])   # {0,1,2,3} and {4,5,6} are one split, and the moved tree lacks it


def unrooted_cases(lib):
    # one unrooted tree on six leaves, ((0,1),2,(3,(4,5))) around its middle node, written with three different last joins
    a = [(0, 1), (4, 5), (3, 7), (6, 2), (9, 8)]
    b = [(0, 1), (4, 5), (3, 7), (2, 8), (6, 9)]
    c = [(4, 5), (0, 1), (7, 2), (8, 6), (3, 9)]
    for main in (a, b, c):
        check(lib, main, [a, b, c], True, [3] * 5)
    got = check(lib, a, [a, b, c], False)
    assert got.tolist() != [3] * 5                          # rooted, the three differ
    # a clade matched only by its complement: main has {0,1,2}; the replicate holds {3,4,5} and never {0,1,2}
    main = [(0, 1), (6, 2), (3, 4), (8, 5), (7, 9)]
    rep = [(3, 4), (6, 5), (0, 7), (8, 1), (9, 2)]
    assert frozenset([0, 1, 2]) not in leaf_sets(rep, 6) and frozenset([3, 4, 5]) in leaf_sets(rep, 6)
    check(lib, main, [rep], True, [0, 1, 1, 1, 1])
    check(lib, main, [rep], False, [0, 0, 1, 1, 1])
    # a split whose sides are both in two pieces once the leaves are numbered along the main tree: rep2 has {2,3,4,5} only as the other
    # side of its node {0,1}, and {2,3} | {0,1,4,5} not at all
    rep2 = [(0, 1), (4, 5), (6, 2), (7, 8), (9, 3)]         # {0,1}, {4,5}, {0,1,2}, {0,1,2,4,5}
    main2 = [(2, 3), (4, 5), (6, 7), (0, 1), (8, 9)]        # {2,3}, {4,5}, {2,3,4,5}, {0,1}
    check(lib, main2, [rep2], True, [0, 1, 1, 1, 1])
    # trivial splits: |L| >= n - 1 gets every replicate; the replicate holds {0,1,2,3} only as the other side of leaf 4
    check(lib, caterpillar(np.arange(5)), [caterpillar(np.array([4, 0, 2, 1, 3]))], True, [0, 0, 1, 1])
    check(lib, caterpillar(np.arange(5)), [caterpillar(np.array([4, 0, 2, 1, 3]))], False, [0, 0, 0, 1])
    check(lib, caterpillar(np.arange(5)), [caterpillar(np.array([4, 3, 2, 1, 0]))], True, [1, 1, 1, 1])     # the same path from its other end


def random_trees(lib):
    rng = np.random.default_rng(11)
    for n in (33, 257):
        order = rng.permutation(n)
        main = split_tree(order, rng)
        reps = [main if r == 0 else rewritten(main, rng) for r in range(2)]
        for r in range(3):                                  # the same order with a few leaves exchanged: many clades stay, some go
            o = order.copy()
            for _ in range(1 + 2 * r):
                i, j = rng.integers(n, size=2)
                o[i], o[j] = o[j], o[i]
            reps.append(split_tree(o, rng) if r else split_tree(order, rng))
        for unrooted in (False, True):
            got = check(lib, main, reps, unrooted)
            assert 2 <= int(got.min()) and int(got.max()) == 5 and len(set(got.tolist())) >= 2, got.tolist()


def deep_caterpillar(lib):
    """65 536 leaves, as deep as wide: no recursion.  The answers are known: itself, and the caterpillar over the reversed order, which shares
    the set of all leaves only (rooted) and every split (unrooted: the same path read from the other end)"""
    n = 65536
    cat, rev = caterpillar(np.arange(n)), caterpillar(np.arange(n)[::-1])
    assert tree_support(cat, [cat], False, lib=lib).tolist() == [1] * (n - 1)
    assert tree_support(cat, [rev], False, lib=lib).tolist() == [0] * (n - 2) + [1]
    assert tree_support(cat, [rev], True, lib=lib).tolist() == [1] * (n - 1)
    # leaf 1 and leaf 2 exchanged: only {0, 1} goes
    order = np.arange(n)
    order[[1, 2]] = order[[2, 1]]
    assert tree_support(cat, [caterpillar(order)], False, lib=lib).tolist() == [0] + [1] * (n - 2)


def support_errors(lib):
    main = np.array([(0, 1), (3, 2)], dtype=np.int32)
    sup = np.zeros(2, dtype=np.uint32)

    def call(ch, n, reps, b, out=sup):
        ch = None if ch is None else np.ascontiguousarray(ch, dtype=np.int32)
        reps = None if reps is None else np.ascontiguousarray(reps, dtype=np.int32)
        return lib.ani_tree_support(None if ch is None else ch.ctypes.data, n, None if reps is None else reps.ctypes.data, b, 0,
                                    None if out is None else out.ctypes.data)

    assert call(main, 3, [main], 1) == 0
    assert call(None, 3, [main], 1) == ERR_ARG and call(main, 3, None, 1) == ERR_ARG and call(main, 3, [main], 1, None) == ERR_ARG
    assert call(main, 3, None, 0) == 0                                     # no replicates: nothing to read
    assert call(main, -1, [main], 1) == ERR_ARG and call(main, 3, [main], -1) == ERR_ARG
    for bad in ([(0, 1), (4, 2)], [(0, 1), (3, 3)], [(0, 3), (3, 2)], [(0, 1), (1, 2)], [(0, 0), (3, 2)], [(0, -1), (3, 2)], [(0, 1), (3, 5)], [(0, 1), (0, 2)]):
        assert call(bad, 3, [main], 1) == ERR_ARG, bad
        assert call(main, 3, [main, bad], 2) == ERR_ARG, bad
    with pytest.raises(AniError) as ex:
        tree_support([(0, 1), (1, 2)], [main], lib=lib)
    assert ex.value.code == ERR_ARG and "not a tree" in str(ex.value)


def test_tree_support_cpu_build(emu_engine):
    lib = emu_engine.lib
    hand_written(lib)
    same_tree_rewritten(lib)
    caterpillar_and_balanced(lib)
    one_clade_moved(lib)
    unrooted_cases(lib)
    random_trees(lib)
    support_errors(lib)


def test_tree_support_deep_cpu_build(emu_engine):
    deep_caterpillar(emu_engine.lib)


@pytest.mark.gpu
def test_tree_support_gpu(gpu_engine):
    """the same host function as the product library holds it"""
    lib = gpu_engine.lib
    hand_written(lib)
    unrooted_cases(lib)
    random_trees(lib)
    support_errors(lib)
    deep_caterpillar(lib)


# ---- the composed call ----
METHODS = ("average", "nj", "single")


def tree_of(engine, method, rows, n, missing=0.0):
    if method == "nj":
        return np.asarray(engine.tree_nj(rows, n, missing)[0], dtype=np.int32)
    z = engine.tree_average(rows, n, missing) if method == "average" else engine.tree_single(rows, n, missing)
    return z[:, 0:2].astype(np.int32)


def flip_rows(n):
    """two groups, {0..3} and {4..n-1}, far apart; the first is (((0,1),2),3); every pair has one row.  The replicate identities are the
    rows' own, with small moves that change no clade, except in replicates 1 and 3, where 0 goes with 2 first and 1 joins the two after"""
    w = {}
    for i in range(n):
        for j in range(i + 1, n):
            a, b = i < 4, j < 4
            w[(i, j)] = 85.0 + 0.01 * (i + j) if a != b else (95.0 + 0.01 * i if a else 96.0 + 0.3 * (j - i) - 0.01 * i)
    w[(0, 1)], w[(0, 2)], w[(1, 2)] = 99.0, 97.0, 97.0
    w[(4, 5)] = 99.2
    keys = sorted(w)
    rows = make_rows([(j, i, np.float32(w[(i, j)])) for i, j in keys])
    rep = np.repeat(rows["identity"].astype(np.float32)[:, None], 5, axis=1)
    rep += np.float32(0.001) * (np.arange(5, dtype=np.float32)[None, :] - 2)
    for r in (1, 3):
        rep[keys.index((0, 1)), r] = 97.0
        rep[keys.index((0, 2)), r] = 99.5
    return rows, np.ascontiguousarray(rep)


def composed(engine):
    for n in (8, 9):
        rows, rep = flip_rows(n)
        for method in METHODS:
            main = tree_of(engine, method, rows, n)
            got = engine.tree_support_bootstrap(method, rows, n, rep, main)
            reps = []
            for r in range(5):
                x = rows.copy()
                x["identity"] = rep[:, r]
                reps.append(tree_of(engine, method, x, n))
            assert got.tolist() == tree_support(main, reps, method == "nj", lib=engine.lib).tolist(), (n, method)
            assert got.tolist() == restated(main, reps, method == "nj").tolist(), (n, method)
            sets = leaf_sets(main, n)
            at = dict((sets[n + s], s) for s in range(n - 1))
            assert frozenset([0, 1, 2]) in at and (frozenset(range(4)) in at or frozenset(range(4, n)) in at), (n, method, sorted(map(sorted, at)))
            # {0,1} is gone in exactly two replicates; every other clade, the split between the two groups among them, is in all five
            assert [int(got[s]) for s in range(n - 1)] == [3 if sets[n + s] == frozenset([0, 1]) else 5 for s in range(n - 1)], (n, method, got.tolist())
            # another main tree than the method's own is taken as it is
            other = caterpillar(np.arange(n))
            assert engine.tree_support_bootstrap(method, rows, n, rep, other).tolist() == restated(other, reps, method == "nj").tolist()
        # no replicates, no rows, one genome
        assert engine.tree_support_bootstrap("average", rows, n, rep[:, :0], main).tolist() == [0] * (n - 1)
    assert engine.tree_support_bootstrap("single", make_rows([]), 1, np.zeros((0, 5), np.float32), np.zeros((0, 2), np.int32)).shape == (0,)
    none = make_rows([])
    main = tree_of(engine, "average", none, 4)
    assert engine.tree_support_bootstrap("average", none, 4, np.zeros((0, 3), np.float32), main).tolist() == [3, 3, 3]


def composed_errors(engine):
    rows, rep = flip_rows(8)
    main = tree_of(engine, "average", rows, 8)

    def refused(code=ERR_ARG, method="average", rows=rows, n=8, rep=rep, children=main, missing=0.0):
        with pytest.raises(AniError) as ex:
            engine.tree_support_bootstrap(method, rows, n, rep, children, missing)
        assert ex.value.code == code, (ex.value.code, code)

    for v in (0.0, -1.0, 100.5, float("nan"), float("inf")):
        bad = rep.copy()
        bad[3, 2] = v
        refused(rep=bad)
    for missing in (-1.0, 100.5, float("nan")):
        refused(missing=missing)
    refused(method=3)
    refused(method=-1)
    bad = rows.copy()
    bad["refGenomeId"][2] = 8
    refused(rows=bad)
    bad = main.copy()
    bad[0] = (0, 0)
    refused(children=bad)
    lib, h = engine.lib, engine.h
    sup = np.zeros(7, np.uint32)
    f0 = ctypes.c_float(0.0)
    args = (rows.ctypes.data, len(rows), 8, f0, rep.ctypes.data, 5)
    assert lib.ani_tree_support_bootstrap(h, 0, *args, main.ctypes.data, sup.ctypes.data) == 0
    assert lib.ani_tree_support_bootstrap(None, 0, *args, main.ctypes.data, sup.ctypes.data) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, *args, None, sup.ctypes.data) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, *args, main.ctypes.data, None) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, None, len(rows), 8, f0, rep.ctypes.data, 5, main.ctypes.data, sup.ctypes.data) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, rows.ctypes.data, len(rows), 8, f0, None, 5, main.ctypes.data, sup.ctypes.data) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, rows.ctypes.data, len(rows), 8, f0, rep.ctypes.data, -1, main.ctypes.data, sup.ctypes.data) == ERR_ARG
    assert lib.ani_tree_support_bootstrap(h, 0, rows.ctypes.data, len(rows), -1, f0, rep.ctypes.data, 5, main.ctypes.data, sup.ctypes.data) == ERR_ARG
    # the tree calls' limits, before anything is read or allocated: 65 537 genomes (not for single), 2^32 rows
    for method, code in ((0, ERR_LIMIT), (1, ERR_LIMIT)):
        assert lib.ani_tree_support_bootstrap(h, method, rows.ctypes.data, 0, 65537, f0, rep.ctypes.data, 0, main.ctypes.data, sup.ctypes.data) == code
    assert lib.ani_tree_support_bootstrap(h, 2, rows.ctypes.data, 0, (1 << 30) + 1, f0, rep.ctypes.data, 0, main.ctypes.data, sup.ctypes.data) == ERR_LIMIT
    assert lib.ani_tree_support_bootstrap(h, 0, rows.ctypes.data, 1 << 32, 8, f0, rep.ctypes.data, 0, main.ctypes.data, sup.ctypes.data) == ERR_LIMIT


# ---- the statistic, on the restatement alone, then the engine held to it ----
STAT_B, STAT_SEED = 100, 1


def statistic_case():
    """five genomes: {0, 1, 2} and {3, 4}.  Within a group the cells are near 97, between the groups near 80; the three pairs of the first
    group have heavily overlapping cells (one distribution, 40 to 42 cells each), so which two of them join first is a matter of the
    sample.  -> rows, replicate identities by the boot records' rules 1 and 3, the UPGMA tree of the rows, the support by the restatement"""
    rng = np.random.default_rng(2)
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    rows, rep = [], []
    for k, (i, j) in enumerate(pairs):
        within = (i < 3) == (j < 3)
        count = 40 + k if within else 60 + k
        x = (rng.normal(97.0, 1.5, count) if within else rng.normal(80.0, 1.0, count)).clip(70.0, 100.0).astype(np.float32)
        if (i, j) == (3, 4):
            x = (x + np.float32(1.5)).clip(70.0, 100.0)
        f = cc.fix(bc.bits(x))
        total, sums = bc.replicate_sums(f, STAT_B, STAT_SEED)
        rec = np.zeros(1, dtype=BOOT_DT)
        rec["count"], rec["sum"] = count, total
        rows.append((j, i, boot_identity(rec, np.array([[total]], dtype=np.uint64))[0, 0]))
        rep.append(boot_identity(rec, sums[None, :])[0])
    rows, rep = make_rows(rows), np.ascontiguousarray(np.stack(rep))
    main = np.asarray(upgma(rows, 5, 0.0)[0], dtype=np.int32).reshape(4, 2)
    reps = []
    for r in range(STAT_B):
        x = rows.copy()
        x["identity"] = rep[:, r]
        reps.append(np.asarray(upgma(x, 5, 0.0)[0], dtype=np.int32).reshape(4, 2))
    return rows, rep, main, restated(main, reps)


def check_statistic(main, support):
    sets = leaf_sets(main, 5)
    at = dict((sets[5 + s], s) for s in range(4))
    assert frozenset([0, 1, 2]) in at and frozenset([3, 4]) in at, sorted(map(sorted, at))
    assert int(support[at[frozenset([0, 1, 2])]]) == STAT_B and int(support[at[frozenset([3, 4])]]) == STAT_B       # the groups: every replicate
    inner = [c for c in at if len(c) == 2 and c < frozenset([0, 1, 2])]
    assert len(inner) == 1 and 1 <= int(support[at[inner[0]]]) <= STAT_B - 1, (inner, support.tolist())              # the contested clade
    return int(support[at[inner[0]]])


def test_statistic_restatement():
    rows, rep, main, support = statistic_case()
    print("the contested clade: %d of %d" % (check_statistic(main, support), STAT_B))


def statistic_engine(engine):
    rows, rep, main, support = statistic_case()
    check_statistic(main, support)
    assert tree_of(engine, "average", rows, 5).tolist() == main.tolist()
    assert engine.tree_support_bootstrap("average", rows, 5, rep, main).tolist() == support.tolist()


def test_composed_cpu_build(emu_engine):
    composed(emu_engine)
    composed_errors(emu_engine)
    statistic_engine(emu_engine)


@pytest.mark.gpu
def test_composed_gpu(gpu_engine):
    composed(gpu_engine)
    composed_errors(gpu_engine)
    statistic_engine(gpu_engine)
