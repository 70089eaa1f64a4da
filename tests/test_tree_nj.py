"""Neighbour-joining tree (ani_tree_nj, Engine.tree_nj, fastANI --tree --treeMethod nj) against a numpy statement of its fixed-point
semantics (include/ani_abi.h, rules 2 - 8), and against a random tree whose additive distances NJ must give back exactly.
CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import orc
from fastani_amd.api import CGI_DT, AniError
from test_cluster import VARIANTS, clique_rows, make_rows, pair_weights, path_rows, random_rows, read_matrix
from test_tree import hub_rows, random_identity_rows, read_name, tree_genomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
UNIT = float(1 << 24)
LIMIT = (1 << 31) - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the semantics, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def leaf_q(n, lo, hi, w, missing):
    """rule 2: int distances in units of 2^-24, q = rint((100 - w) 2^24 / 100) in double (numpy's rint rounds half to even)"""
    qm = np.rint((100.0 - np.float64(np.float32(missing))) * UNIT / 100.0).astype(np.int64)
    q = np.full((n, n), qm, dtype=np.int64)
    x = np.rint((100.0 - w.astype(np.float64)) * UNIT / 100.0).astype(np.int64)
    q[lo, hi] = x
    q[hi, lo] = x
    np.fill_diagonal(q, 0)
    return q


def nj_simple(q, margins=None):
    """rules 3 - 8 with the full argmin at every join -> children int64 (n - 1, 2), lengths float32 (n - 1, 2).
    margins (a list): per join with m >= 4, the smallest Q of another pair minus the Q of the pair taken"""
    n = len(q)
    q = q.copy()
    ids = np.arange(n)
    active = np.ones(n, dtype=bool)
    children = np.zeros((max(n - 1, 0), 2), dtype=np.int64)
    length = np.zeros((max(n - 1, 0), 2), dtype=np.float32)
    for s in range(n - 1):
        act = np.flatnonzero(active)
        m = len(act)
        if m > 2:
            sub = q[np.ix_(act, act)]
            r = sub.sum(axis=1)                                     # (the diagonal holds 0)
            crit = (m - 2) * sub - r[:, None] - r[None, :]
            crit[np.tril_indices(m)] = np.iinfo(np.int64).max
            i, j = divmod(int(np.argmin(crit)), m)                  # row-major: the smallest a, then the smallest b
            if margins is not None and m >= 4:
                best = crit[i, j]
                crit[i, j] = np.iinfo(np.int64).max
                margins.append(int(crit.min() - best))
            a, b = int(act[i]), int(act[j])
            t = np.float64(int(r[i] - r[j])) / np.float64(m - 2)
            la = np.float32((np.float64(q[a, b]) + t) * 0.5 / UNIT)
            lb = np.float32((np.float64(q[a, b]) - t) * 0.5 / UNIT)
        else:
            a, b = int(act[0]), int(act[1])
            la = lb = np.float32(np.float64(q[a, b]) * 0.5 / UNIT)
        if ids[a] < ids[b]:
            children[s], length[s] = (ids[a], ids[b]), (la, lb)
        else:
            children[s], length[s] = (ids[b], ids[a]), (lb, la)
        if m > 2:
            k = active.copy()
            k[[a, b]] = False
            new = np.clip((q[a, k] + q[b, k] - q[a, b]) >> 1, -LIMIT, LIMIT)      # >> on int64: arithmetic, floor
            q[a, k] = new
            q[k, a] = new
            active[b] = False
            ids[a] = n + s
    return children, length


def expected(rows, n, missing, margins=None):
    return nj_simple(leaf_q(n, *pair_weights(rows), missing), margins)


def check(engine, rows, n, missing=0.0):
    children, length = engine.tree_nj(rows, n, missing)
    want_c, want_l = expected(rows, n, missing)
    m = max(n - 1, 0)
    assert children.dtype == np.int64 and children.shape == (m, 2) and length.dtype == np.float32 and length.shape == (m, 2)
    bad = np.nonzero((children != want_c).any(axis=1) | (length.view(np.uint32) != want_l.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (n, bad[:5], children[bad[:5]], want_c[bad[:5]], length[bad[:5]], want_l[bad[:5]])
    if m:
        assert (children[:, 0] < children[:, 1]).all()
        assert sorted(children.ravel().tolist()) == list(range(2 * n - 2))       # every node but the last is a child exactly once
        if n >= 3:
            assert 2 * n - 3 in children[-1]                                     # rule 7
    return children, length


# ---------------------------------------------------------------------------------------------------------------------------------
# the API against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    rows = make_rows([(0, 1, 97.0), (1, 2, 96.0)])
    for missing in (-1.0, 100.5, float("nan")):
        with pytest.raises(AniError) as ex:
            engine.tree_nj(rows, 3, missing)
        assert ex.value.code == -1, missing                            # ANI_ERR_ARG
    for bad in ((0, 3, 97.0), (-1, 1, 97.0), (2, 5, 97.0), (0, 2, 0.0), (0, 2, -3.0), (0, 2, 100.5), (1, 1, float("nan")), (0, 1, float("inf"))):
        with pytest.raises(AniError) as ex:
            engine.tree_nj(make_rows([(0, 1, 97.0), bad]), 3)
        assert ex.value.code == -1, bad
    with pytest.raises(AniError) as ex:
        engine.tree_nj(rows, -1)
    assert ex.value.code == -1
    ch, ln = np.zeros(4, np.int32), np.zeros(4, np.float32)
    assert engine.lib.ani_tree_nj(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), None, ln.ctypes.data) == -1
    assert engine.lib.ani_tree_nj(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, None) == -1
    assert engine.lib.ani_tree_nj(engine.h, None, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, ln.ctypes.data) == -1
    # limits, before anything is allocated or read: 65 537 genomes, 2^32 rows
    assert engine.lib.ani_tree_nj(engine.h, rows.ctypes.data, 2, 65537, ctypes.c_float(0.0), ch.ctypes.data, ln.ctypes.data) == -4
    assert engine.lib.ani_tree_nj(engine.h, rows.ctypes.data, 1 << 32, 3, ctypes.c_float(0.0), ch.ctypes.data, ln.ctypes.data) == -4
    # n <= 1: nothing to join, nothing written
    for n in (0, 1):
        c, l = engine.tree_nj(make_rows([]), n)
        assert c.shape == (0, 2) and l.shape == (0, 2)
    assert engine.tree_nj(make_rows([(0, 0, 100.0)]), 1)[0].shape == (0, 2)
    ch[:], ln[:] = -7, -7.0
    assert engine.lib.ani_tree_nj(engine.h, None, 0, 1, ctypes.c_float(0.0), None, None) == 0
    assert engine.lib.ani_tree_nj(engine.h, rows.ctypes.data, 2, 1, ctypes.c_float(0.0), ch.ctypes.data, ln.ctypes.data) == 0
    assert (ch == -7).all() and (ln == -7.0).all()
    # missing identity 0 and 100 are both allowed
    check(engine, rows, 3, 100.0)


def small_inputs(engine, seed):
    rng = np.random.default_rng(seed)
    # n = 2, 3, 4 with and without rows
    c, l = check(engine, make_rows([]), 2)
    assert c.tolist() == [[0, 1]] and l.tolist() == [[0.5, 0.5]]
    check(engine, make_rows([(1, 0, 97.5)]), 2)
    check(engine, make_rows([(0, 1, 99.0), (2, 1, 90.0)]), 3)
    check(engine, make_rows([(0, 1, 99.0), (2, 1, 90.0), (0, 2, 91.0)]), 3, 75.0)
    check(engine, make_rows([(0, 3, 99.0), (2, 1, 98.0), (0, 2, 91.0), (1, 3, 90.5)]), 4)
    check(engine, make_rows([]), 3)
    check(engine, make_rows([]), 4)
    # no rows at all: every Q ties at every join, the tie rule alone decides
    c, _ = check(engine, make_rows([]), 9)
    assert c[0].tolist() == [0, 1]
    check(engine, make_rows([]), 9, 75.0)
    check(engine, make_rows([]), 70)
    # fold order: the result depends on the order given; self rows ignored
    rows = make_rows([(1, 0, 94.0), (0, 1, 96.5), (1, 0, 95.25), (2, 3, 95.0), (3, 2, 94.999), (4, 4, 100.0), (0, 2, 90.0)])
    check(engine, rows, 7)
    check(engine, rows[::-1].copy(), 7)
    check(engine, rows, 7, 75.0)
    # 12 ... 130 genomes: 65 = just above a multiple of 64, 100 = no multiple; every size above 73 is compacted at least once
    for n, pairs in ((12, 40), (65, 500), (100, 700), (130, 900)):
        check(engine, random_identity_rows(rng, n, pairs), n)
        check(engine, random_identity_rows(rng, n, pairs), n, 75.0)
        check(engine, random_identity_rows(rng, n, pairs, integer=True), n)       # integer identities: many equal distances
        check(engine, random_rows(rng, n, pairs, 95.0), n + 3)                    # several rows per pair in both orders, self rows
    check(engine, clique_rows(rng, 70, 95.0), 70)
    check(engine, path_rows(100, 95.0), 100)
    check(engine, hub_rows(90), 90)
    check(engine, hub_rows(90), 90, 85.0)


def test_nj_api_cpu_build(emu_engine):
    argument_errors(emu_engine)
    small_inputs(emu_engine, 1)


@pytest.mark.gpu
def test_nj_api_gpu(gpu_engine):
    argument_errors(gpu_engine)
    small_inputs(gpu_engine, 2)
    rng = np.random.default_rng(3)
    # 1100 = 4 tiles of 256 columns and a part of a fifth, 1025 = just above a multiple of 64; the restatement is the slow side
    check(gpu_engine, random_identity_rows(rng, 1100, 30000), 1100)
    check(gpu_engine, random_identity_rows(rng, 1025, 30000, integer=True), 1025, 75.0)
    check(gpu_engine, random_rows(rng, 600, 20000, 95.0), 600)
    check(gpu_engine, make_rows([]), 520)
    check(gpu_engine, clique_rows(rng, 500, 95.0), 500)
    check(gpu_engine, path_rows(700, 95.0), 700)
    check(gpu_engine, hub_rows(640), 640)


@pytest.mark.gpu
def test_nj_large_matrix_gpu(gpu_engine):
    """5000 genomes: 64-row tiles, more tiles than workgroups, a dozen compactions.  Too large for the restatement, so what is checked
    is what any neighbour-joining run must give: every node a child exactly once, and the records of an input with one close pair per
    leaf-disjoint couple (2k, 2k + 1) join exactly those couples first."""
    n = 5000
    pairs = [(2 * k, 2 * k + 1, 99.0) for k in range(n // 2)]
    rows = make_rows(pairs)
    children, length = gpu_engine.tree_nj(rows, n, 50.0)
    assert sorted(children.ravel().tolist()) == list(range(2 * n - 2))
    assert 2 * n - 3 in children[-1]
    leaf_joins = {tuple(c) for c in children.tolist() if c[1] < n}
    assert leaf_joins == {(2 * k, 2 * k + 1) for k in range(n // 2)}
    first = children[:, 1] < n
    assert np.array_equal(length[first], np.full((n // 2, 2), np.float32(167772 * 0.5 / UNIT)))      # q = rint(0.01 * 2^24), t = 0 by symmetry


@pytest.mark.gpu
def test_nj_rows_of_the_engine_gpu(gpu_engine):
    """rows from the mapping path itself (Sketch.map_cgi_batch over synthetic species clusters), treed"""
    import fastani_amd
    e = gpu_engine
    p = e.params(16, 3000)
    genomes = [[orc.synth_genome(13, g, 120000)] for g in list(range(0, 12)) + list(range(20, 30)) + [40, 41, 60]]
    sk = fastani_amd.Sketch(e, p, genomes)
    rows = sk.map_cgi_batch(genomes, 0)
    assert len(rows) > 100
    check(e, rows, len(genomes))
    check(e, rows, len(genomes), 75.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# additive distances give the tree back exactly
# ---------------------------------------------------------------------------------------------------------------------------------
def random_tree(rng, n_leaves):
    """a random rooted binary tree grown by splitting a random leaf, the most recent ones preferred (so the tree is lopsided: leaf depths
    differ widely), edges of length 1 - 3 -> parent, edge length per node; the leaves are nodes relabelled 0..n_leaves-1 at random"""
    parent, edge, leaves = [-1], [0], [0]
    while len(leaves) < n_leaves:
        i = int(rng.integers(max(0, len(leaves) - 6), len(leaves)))
        v = leaves.pop(i)
        for _ in range(2):
            parent.append(v)
            edge.append(int(rng.integers(1, 4)))
            leaves.append(len(parent) - 1)
    return np.array(parent), np.array(edge), rng.permutation(np.array(leaves))


def tree_paths(parent, edge, leaves):
    """-> path length T(i, j) between leaves, depth of every leaf, {split: edge length} over the non-trivial and trivial splits of the
    unrooted tree (the two edges at the root are one edge: their sum)"""
    n_nodes, n = len(parent), len(leaves)
    depth = np.zeros(n_nodes, dtype=np.int64)
    for v in range(1, n_nodes):                                     # a parent's index is below its children's
        depth[v] = depth[parent[v]] + edge[v]
    below = np.zeros((n_nodes, n), dtype=bool)
    below[leaves, np.arange(n)] = True
    for v in range(n_nodes - 1, 0, -1):
        below[parent[v]] |= below[v]
    # T(i, j) = depth_i + depth_j - 2 depth(lca): the lca is the deepest node above both
    T = np.zeros((n, n), dtype=np.int64)
    lca_depth = np.zeros((n, n), dtype=np.int64)
    for v in np.argsort(depth, kind="stable"):                      # deeper nodes overwrite shallower ones
        idx = np.flatnonzero(below[v])
        lca_depth[np.ix_(idx, idx)] = depth[v]
    d = depth[leaves]
    T = d[:, None] + d[None, :] - 2 * lca_depth
    np.fill_diagonal(T, 0)
    everyone = frozenset(range(n))
    splits = {}
    for v in range(1, n_nodes):
        side = frozenset(np.flatnonzero(below[v]).tolist())
        key = frozenset([side, everyone - side])
        splits[key] = splits.get(key, 0) + int(edge[v])
    return T, d, splits


def splits_of(children, length, n):
    """the unrooted tree of the records -> {split: branch length (float64 of the float32s; the last record's two are one edge)}"""
    everyone = frozenset(range(n))
    clade = [frozenset([i]) for i in range(n)]
    out = {}
    for s, (x, y) in enumerate(children.tolist()):
        clade.append(clade[x] | clade[y])
        if s == len(children) - 1:
            out[frozenset([clade[x], clade[y]])] = float(length[s, 0]) + float(length[s, 1])
            assert clade[x] | clade[y] == everyone
        else:
            for c, l in ((x, length[s, 0]), (y, length[s, 1])):
                out[frozenset([clade[c], everyone - clade[c]])] = float(l)
    return out


def additive(engine):
    """256 leaves, w = 100 - 25 T / 256 (exact in float32), so q = T 2^14 exactly: every Q, every halving and every branch is exact
    and neighbour joining must return the tree itself, each branch edge / 1024.  Average linkage cannot: the tree is far from
    clock-like (asserted: the leaf depths spread over more than a factor of two), and it joins by distance alone."""
    rng = np.random.default_rng(11)
    n = 256
    parent, edge, leaves = random_tree(rng, n)
    T, depth, truth = tree_paths(parent, edge, leaves)
    assert depth.max() > 2 * depth.min() and T.max() < 1024, (depth.min(), depth.max(), T.max())
    a, b = np.triu_indices(n, 1)
    rows = np.zeros(len(a), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = b, a
    rows["identity"] = (100.0 - 25.0 * T[a, b] / 256.0).astype(np.float32)
    assert np.array_equal(rows["identity"].astype(np.float64), 100.0 - 25.0 * T[a, b] / 256.0)
    children, length = engine.tree_nj(rows, n, 0.0)
    got = splits_of(children, length, n)
    assert len(truth) == 2 * n - 3
    assert set(got) == set(truth)
    for k, e in truth.items():
        assert got[k] == e / 1024.0, (sorted(min(k, key=len)), got[k], e)
    # the same rows through average linkage: other splits
    z = engine.tree_average(rows, n, 0.0)
    clade = [frozenset([i]) for i in range(n)]
    everyone = frozenset(range(n))
    upgma = set()
    for x, y in z[:, :2].astype(np.int64).tolist():
        clade.append(clade[x] | clade[y])
        upgma.add(frozenset([clade[-1], everyone - clade[-1]]))
    nontrivial = {k for k in truth if min(len(s) for s in k) > 1}
    assert len(nontrivial) == n - 3
    assert not nontrivial <= upgma, "average linkage found every split: the tree is too clock-like to tell the methods apart"


def test_nj_additive_tree_cpu_build(emu_engine):
    additive(emu_engine)


@pytest.mark.gpu
def test_nj_additive_tree_gpu(gpu_engine):
    additive(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# a negative branch, and the clamp
# ---------------------------------------------------------------------------------------------------------------------------------
def negative_branch(engine):
    """Four genomes, the pair {1, 3} without rows (identity 0: q = 2^24 = U), q(0,1) = q(0,2) = q(2,3) = U/4 (identity 75),
    q(0,3) = q(1,2) = U/2 (identity 50).  R = (U, 7U/4, U, 7U/4), m = 4:
      Q(0,1) = U/2 - 11U/4 = -9U/4   Q(0,2) = U/2 - 2U = -3U/2   Q(0,3) = U - 11U/4 = -7U/4
      Q(1,2) = U - 11U/4 = -7U/4     Q(1,3) = 2U - 7U/2 = -3U/2  Q(2,3) = U/2 - 11U/4 = -9U/4
    Q(0,1) = Q(2,3) is the smallest; the tie goes to (0, 1).  t = (U - 7U/4) / 2 = -3U/8:
      len_0 = (U/4 - 3U/8) / 2 / U = -1/16 (negative: 1 is far from 3, 0 is not)   len_1 = (U/4 + 3U/8) / 2 / U = 5/16.
    Node 4 = {0, 1} in slot 0: q(4,2) = (U/4 + U/2 - U/4) / 2 = U/4, q(4,3) = (U/2 + U - U/4) / 2 = 5U/8.  R = (7U/8, -, U/2, 7U/8), m = 3:
    every Q = -(U/4 + 5U/8 + U/4) = -9U/8, the tie goes to slots (0, 2) = nodes (4, 2): t = 3U/8,
      len_4 = (U/4 + 3U/8) / 2 / U = 5/16   len_2 = (U/4 - 3U/8) / 2 / U = -1/16.
    Node 5 in slot 0: q(5,3) = (5U/8 + U/4 - U/4) / 2 = 5U/16; the last record (3, 5) has 5/32 on either side."""
    rows = make_rows([(0, 1, 75.0), (0, 2, 75.0), (2, 3, 75.0), (0, 3, 50.0), (1, 2, 50.0)])
    children, length = check(engine, rows, 4)
    assert children.tolist() == [[0, 1], [2, 4], [3, 5]]
    assert length.tolist() == [[-0.0625, 0.3125], [-0.0625, 0.3125], [0.15625, 0.15625]]
    # the clamp of rule 6 cannot be reached from identities in (0, 100] (q <= 2^24), so the update is checked at the other end:
    # q(0,2) = q(1,2) = 0 and q(0,1) = U give q(new, 2) = -U/2, a negative distance kept as it is
    children, length = check(engine, make_rows([(0, 2, 100.0), (1, 2, 100.0)]), 3)
    assert children.tolist() == [[0, 1], [2, 3]] and length.tolist() == [[0.5, 0.5], [-0.25, -0.25]]


def test_nj_negative_branch_cpu_build(emu_engine):
    negative_branch(emu_engine)


@pytest.mark.gpu
def test_nj_negative_branch_gpu(gpu_engine):
    negative_branch(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def parse_unrooted(text):
    """'(A:x,B:y,C:z);' over binary subtrees -> {clade (frozenset of leaf names): branch length}, the clades at the top"""
    assert text.endswith(";\n")
    s = text[:-2]
    lengths, stack, last, i, item = {}, [[]], None, 0, True     # item: a name or a bracket comes next
    while i < len(s):
        c = s[i]
        assert item == (c not in ",):"), (i, s[max(0, i - 20):i + 20])
        if c == "(":
            stack.append([])
            i += 1
        elif c == ",":
            item = True
            i += 1
        elif c == ")":
            kids = stack.pop()
            assert len(kids) == (2 if len(stack) > 1 else len(kids)), kids
            last = frozenset().union(*kids)
            stack[-1].append(last)
            if len(stack) == 1:
                top = kids
            i += 1
        elif c == ":":
            j = i + 1
            while j < len(s) and s[j] not in ",)":
                j += 1
            assert last not in lengths
            lengths[last] = float(s[i + 1:j])
            i = j
        else:
            name, i = read_name(s, i)
            last = frozenset([name])
            stack[-1].append(last)
            item = False
    assert i == len(s) and len(stack) == 1 and len(stack[0]) == 1
    return lengths, top


def nj_from_matrix(path):
    """the restatement over the printed .matrix values -> {split of the names: branch length}, the margins of its joins"""
    names, cells = read_matrix(path)
    n = len(names)
    keys = sorted(cells)
    rows = make_rows([(j, i, np.float32(cells[(j, i)])) for j, i in keys])
    margins = []
    children, length = expected(rows, n, 0.0, margins)
    return {frozenset(frozenset(names[i] for i in side) for side in k): v for k, v in splits_of(children, length, n).items()}, margins


def run_cli(binary, tmp, n_len, variants=()):
    lst = tree_genomes(tmp, n_len)
    names = [x for x in open(lst).read().split("\n") if x]
    n = len(names)
    base = os.path.join(tmp, "plain.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "-o", base], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    # --treeMethod average is --tree alone
    avg = os.path.join(tmp, "avg.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "--treeMethod", "average", "-o", avg], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for ext in ("", ".matrix", ".newick"):
        assert open(avg + ext, "rb").read() == open(base + ext, "rb").read(), ext
    out = os.path.join(tmp, "nj.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "--treeMethod", "nj", "-o", out], capture_output=True,
                       env=dict(os.environ, ANI_CLI_TRACE="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"tree written" in r.stderr
    assert open(out, "rb").read() == open(base, "rb").read()                           # -o and .matrix unchanged
    assert open(out + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    text = open(out + ".newick").read()
    assert text != open(base + ".newick").read()
    quoted = [x for x in names if x.endswith((",1.fa", "[y].fa"))]
    assert len(quoted) == 2
    for x in quoted:
        assert "'%s':" % x.replace("'", "''") in text
    got, top = parse_unrooted(text)
    assert len(top) == 3 and frozenset().union(*top) == frozenset(names)               # one trifurcation over binary subtrees
    assert len(got) == 2 * n - 3
    everyone = frozenset(names)
    got = {frozenset([c, everyone - c]): v for c, v in got.items()}
    assert len(got) == 2 * n - 3
    want, margins = nj_from_matrix(base + ".matrix")
    # A printed cell is within 5e-7 of the identity, so q moves by at most one unit (2^24 / 100 * 5e-7 < 0.1, then the rounding) and
    # a Q of m slots by at most (m - 2) + 2 (m - 1) < 3 n units.  Every join with a choice (m >= 4; at m = 3 all three Q are equal by
    # construction, whatever the values) is decided by at least a thousand times that, or is an exact tie between cells that are all
    # "no ANI" (margin 0: the same tie for printed and unprinted values).
    assert all(x == 0 or x > 3000 * n for x in margins), margins
    assert any(x > 0 for x in margins)
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6, (sorted(min(k, key=len)), got[k], want[k])
    # the same tree through the other paths of the command line
    for name, args in variants:
        o = os.path.join(tmp, "v_%s.out" % name)
        r = subprocess.run([binary] + [a.replace("@L", lst).replace("@T", tmp) for a in args] + ["--tree", "--treeMethod", "nj", "-o", o],
                           capture_output=True)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert open(o + ".newick").read() == text, name
    # argument errors
    for args, msg in ((["--treeMethod", "nj"], b"--treeMethod needs --tree"), (["--tree", "--treeMethod", "foo"], b"--treeMethod takes average or nj")):
        o = os.path.join(tmp, "bad.out")
        r = subprocess.run([binary, "--ql", lst, "--rl", lst] + args + ["-o", o], capture_output=True)
        assert r.returncode == 1 and b"ERROR, " + msg in r.stderr, (args, r.returncode, r.stderr[-500:])
        assert not os.path.exists(o + ".newick")
    # two genomes: no trifurcation
    two = os.path.join(tmp, "two.out")
    r = subprocess.run([binary, "-q", names[0], "-r", names[2], "--tree", "--treeMethod", "nj", "-o", two], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got, top = parse_unrooted(open(two + ".newick").read())
    assert len(top) == 2 and set(got) == {frozenset([names[0]]), frozenset([names[2]])}
    assert len(set(got.values())) == 1 and 0 < list(got.values())[0] < 0.2
    return text


def test_cli_nj_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 30000, VARIANTS)


def test_cli_nj_single_genome_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    p = os.path.join(str(tmp_path), "one genome.fa")
    orc.write_fasta(p, [orc.synth_genome(17, 0, 30000)], names=["x"])
    out = os.path.join(str(tmp_path), "one.out")
    r = subprocess.run([os.path.join(EMU, "fastANI_emu"), "-q", p, "-r", p, "--tree", "--treeMethod", "nj", "-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out + ".newick").read() == "'%s';\n" % p


@pytest.mark.gpu
def test_cli_nj_gpu(tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, str(tmp_path), 200000, VARIANTS)
