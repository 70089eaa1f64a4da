"""Single-linkage tree and minimum spanning tree (ani_tree_single, Engine.tree_single, fastANI --tree --treeMethod single) against a
plain-Python statement of their semantics.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product
library and fastani_amd/fastANI."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import orc
from fastani_amd.api import CGI_DT, AniError
from test_cluster import VARIANTS, clique_rows, make_rows, pair_weights, path_rows, random_rows, read_matrix
from test_tree import hub_rows, parse_newick, random_identity_rows, tree_genomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the semantics, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def missing_distance(missing):
    return np.float32(1.0 - np.float64(missing) / 100.0)


def leaf_distances(w, missing):
    """rule 2: d = min((float)(1 - (double)w / 100), dm)"""
    return np.minimum((1.0 - w.astype(np.float64) / 100.0).astype(np.float32), missing_distance(missing))


class Linkage:
    """a union-find that records merges in scipy form, with the leaf pair that caused each"""
    def __init__(self, n):
        self.n, self.up, self.id = n, list(range(n)), list(range(n))
        self.children, self.height, self.edges = [], [], []

    def find(self, x):
        up = self.up
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    def merge(self, lo, hi, d):
        a, b = self.find(lo), self.find(hi)
        if a == b:
            return False
        self.children.append(sorted((self.id[a], self.id[b])))
        self.height.append(d)
        self.edges.append((lo, hi))
        self.up[b] = a
        self.id[a] = self.n + len(self.children) - 1
        return True

    def result(self):
        m = max(self.n - 1, 0)
        assert len(self.children) == m
        return (np.array(self.children, dtype=np.int64).reshape(m, 2), np.array(self.height, dtype=np.float32),
                np.array(self.edges, dtype=np.int64).reshape(m, 2))


def kruskal(link, lo, hi, d):
    """rule 3 over the pairs given: ascending (bits(d), lo, hi)"""
    order = np.lexsort((hi, lo, d.view(np.uint32)))
    for a, b, x in zip(lo[order].tolist(), hi[order].tolist(), d[order]):
        link.merge(a, b, x)


def single_dense(n, lo, hi, w, missing):
    """rules 2-4 over all n (n - 1) / 2 pairs"""
    dm = missing_distance(missing)
    mat = np.full((n, n), dm, dtype=np.float32)
    mat[lo, hi] = leaf_distances(w, missing)
    a, b = np.triu_indices(n, 1)
    link = Linkage(n)
    kruskal(link, a, b, mat[a, b])
    return link.result()


def single_sparse(n, lo, hi, w, missing):
    """rule 5: the pairs with rows below dm only, then the joins to leaf 0"""
    dm = missing_distance(missing)
    d = leaf_distances(w, missing)
    real = d.view(np.uint32) < dm.view(np.uint32)
    link = Linkage(n)
    kruskal(link, lo[real], hi[real], d[real])
    for k in range(1, n):
        link.merge(0, k, dm)
    return link.result()


def expected(rows, n, missing):
    return single_sparse(n, *pair_weights(rows), missing)


def leafsets(children, n):
    sets = [frozenset([i]) for i in range(n)]
    for x, y in children:
        sets.append(sets[int(x)] | sets[int(y)])
    return sets[n:]


def cut(children, height, n, at):
    """the clusters of the linkage cut at height `at` (merges at or below it) -> a label per leaf: its cluster's smallest leaf"""
    link = Linkage(n)
    leaf = list(range(n))                                            # a leaf of every cluster id
    for (x, y), h in zip(children.tolist(), height.tolist()):
        if np.float32(h) <= at:
            link.merge(leaf[x], leaf[y], h)
        leaf.append(leaf[x])
    return components_of(link, n)


def components_of(link, n):
    label = {}
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        out[i] = label.setdefault(link.find(i), i)
    return out


def check(engine, rows, n, missing=0.0):
    z, edges = engine.tree_single(rows, n, missing, return_edges=True)
    children, height, want_edges = expected(rows, n, missing)
    m = max(n - 1, 0)
    assert z.dtype == np.float64 and z.shape == (m, 4)
    assert edges.dtype == np.int64 and edges.shape == (m, 2)
    got_c = z[:, :2].astype(np.int64)
    got_h = z[:, 2].astype(np.float32)
    assert np.array_equal(got_h.astype(np.float64), z[:, 2])         # float32 heights, exact in float64
    bad = np.nonzero((got_c != children).any(axis=1) | (got_h.view(np.uint32) != height.view(np.uint32)) | (edges != want_edges).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got_c[bad[:5]], children[bad[:5]], got_h[bad[:5]], height[bad[:5]], edges[bad[:5]], want_edges[bad[:5]])
    assert (np.diff(got_h) >= 0).all()
    rounds = engine.tree_single_rounds()
    assert 0 <= rounds <= math.ceil(math.log2(max(n, 2))) + 1, rounds
    assert np.array_equal(engine.tree_single(rows, n, missing), z)    # without the edges: the same linkage
    if m:
        count = np.ones(n + m)
        for s in range(m):
            count[n + s] = count[children[s, 0]] + count[children[s, 1]]
        assert np.array_equal(z[:, 3], count[n:])
        hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
        assert hierarchy.is_valid_linkage(z)
    return z, edges


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against itself: rule 5's claim
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatements_agree():
    rng = np.random.default_rng(5)
    inputs = [(random_identity_rows(rng, 60, 400), 60), (random_identity_rows(rng, 80, 300, integer=True), 80),
              (random_identity_rows(rng, 50, 900, integer=True), 50), (random_rows(rng, 70, 500, 95.0), 75), (make_rows([]), 20),
              (clique_rows(rng, 40, 95.0), 40), (path_rows(60, 95.0), 60), (hub_rows(40), 40)]
    for rows, n in inputs:
        for missing in (0.0, 75.0, 100.0):
            lo, hi, w = pair_weights(rows)
            c1, h1, e1 = single_dense(n, lo, hi, w, missing)
            c2, h2, e2 = single_sparse(n, lo, hi, w, missing)
            assert np.array_equal(c1, c2) and np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(e1, e2), (n, missing)
            assert (np.diff(h1) >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    rows = make_rows([(0, 1, 97.0), (1, 2, 96.0)])
    for missing in (-1.0, 100.5, float("nan")):
        with pytest.raises(AniError) as ex:
            engine.tree_single(rows, 3, missing)
        assert ex.value.code == -1, missing                            # ANI_ERR_ARG
    for bad in ((0, 3, 97.0), (-1, 1, 97.0), (2, 5, 97.0), (0, 2, 0.0), (0, 2, -3.0), (0, 2, 100.5), (1, 1, float("nan")), (0, 1, float("inf"))):
        with pytest.raises(AniError) as ex:
            engine.tree_single(make_rows([(0, 1, 97.0), bad]), 3)
        assert ex.value.code == -1, bad
        with pytest.raises(AniError) as ex:                            # the rows are checked whatever the missing identity leaves of them
            engine.tree_single(make_rows([(0, 1, 97.0), bad]), 3, 100.0)
        assert ex.value.code == -1, bad
    with pytest.raises(AniError) as ex:
        engine.tree_single(rows, -1)
    assert ex.value.code == -1
    ch, h, ed = np.zeros(4, np.int32), np.zeros(2, np.float32), np.zeros(4, np.int32)
    f = engine.lib.ani_tree_single
    assert f(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), None, h.ctypes.data, ed.ctypes.data) == -1
    assert f(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, None, ed.ctypes.data) == -1
    assert f(engine.h, None, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data, ed.ctypes.data) == -1
    assert f(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data, None) == 0      # edges may be null
    # 2^32 rows: ANI_ERR_LIMIT before anything is read or allocated
    assert f(engine.h, rows.ctypes.data, 1 << 32, 3, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data, ed.ctypes.data) == -4
    # no 65 536 ceiling: 65 537 genomes, two of them with rows
    z, edges = check(engine, rows, 65537)
    assert z[:2, :2].tolist() == [[0.0, 1.0], [2.0, 65537.0]] and edges[-1].tolist() == [0, 65536] and z[-1, 2] == 1.0
    # n <= 1: nothing to merge, nothing written
    for n in (0, 1):
        assert engine.tree_single(make_rows([]), n).shape == (0, 4)
        z, edges = engine.tree_single(make_rows([]), n, return_edges=True)
        assert z.shape == (0, 4) and edges.shape == (0, 2)
    assert engine.tree_single(make_rows([(0, 0, 100.0)]), 1).shape == (0, 4)
    assert f(engine.h, None, 0, 1, ctypes.c_float(0.0), None, None, None) == 0
    # missing identity 0 and 100 are both allowed; at 100 every merge is a join to leaf 0 at height 0
    z, edges = check(engine, rows, 3, 100.0)
    assert z[:, 2].tolist() == [0.0, 0.0] and edges.tolist() == [[0, 1], [0, 2]]


def small_inputs(engine, seed):
    rng = np.random.default_rng(seed)
    # n = 2 with and without rows; no rows at all (every distance 1: joins to leaf 0)
    z, edges = check(engine, make_rows([]), 2)
    assert z.tolist() == [[0.0, 1.0, 1.0, 2.0]] and edges.tolist() == [[0, 1]]
    check(engine, make_rows([(1, 0, 97.5)]), 2)
    z, edges = check(engine, make_rows([]), 9)
    assert edges.tolist() == [[0, k] for k in range(1, 9)]
    check(engine, make_rows([]), 9, 75.0)
    # fold order: the result depends on the order given; self rows ignored
    rows = make_rows([(1, 0, 94.0), (0, 1, 96.5), (1, 0, 95.25), (2, 3, 95.0), (3, 2, 94.999), (4, 4, 100.0), (0, 2, 90.0)])
    za, _ = check(engine, rows, 7)
    zb, _ = check(engine, rows[::-1].copy(), 7)
    assert not np.array_equal(za[:, 2], zb[:, 2])
    check(engine, rows, 7, 75.0)
    # the clamp: a pair with a row at or beyond the missing distance is a pair without rows
    check(engine, make_rows([(0, 1, 70.0), (1, 2, 75.0), (2, 3, 75.5), (0, 3, 99.0)]), 5, 75.0)
    for n, pairs in ((12, 40), (70, 500), (130, 700)):
        check(engine, random_identity_rows(rng, n, pairs), n)
        check(engine, random_identity_rows(rng, n, pairs), n, 75.0)
        check(engine, random_identity_rows(rng, n, pairs, integer=True), n)       # integer identities: many equal distances
        check(engine, random_identity_rows(rng, n, pairs, integer=True), n, 90.0)
        check(engine, random_rows(rng, n, pairs, 95.0), n + 3)                    # several rows per pair in both orders, self rows
    check(engine, clique_rows(rng, 70, 95.0), 70)
    check(engine, path_rows(100, 95.0), 100)
    check(engine, hub_rows(90), 90)
    check(engine, hub_rows(90), 90, 85.0)


def matches_scipy(engine, seed):
    """tie-free random complete distances: scipy's single linkage merges the same leaf sets at exactly the same heights (single linkage
    only takes minima of the float32 values)"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(seed)
    n = 120
    a, b = np.triu_indices(n, 1)
    rows = np.zeros(len(a), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = a, b
    rows["identity"] = (70 + 30 * (rng.permutation(len(a)) + 0.5) / len(a)).astype(np.float32)    # distinct, 0.004 apart: no two distances equal
    d = leaf_distances(rows["identity"], 0.0)
    assert len(np.unique(d)) == len(d)
    got, _ = check(engine, rows, n)
    z = hierarchy.linkage(d.astype(np.float64), method="single")
    assert leafsets(got[:, :2].astype(np.int64), n) == leafsets(z[:, :2].astype(np.int64), n)
    assert np.array_equal(got[:, 2], z[:, 2])


def properties(engine, seed, sizes):
    """identities on a grid of 0.25 that holds T: the cut of the linkage at (float)(1 - T / 100) is the connected components of the pairs
    with w >= T, and every greedy cluster lies inside one of them"""
    rng = np.random.default_rng(seed)
    for n, pairs, t in sizes:
        rows = random_rows(rng, n, pairs, t)
        z, _ = check(engine, rows, n + 5)
        lo, hi, w = pair_weights(rows)
        link = Linkage(n + 5)
        for a, b in zip(lo[w >= np.float32(t)].tolist(), hi[w >= np.float32(t)].tolist()):
            link.merge(a, b, 0.0)
        want = components_of(link, n + 5)
        got = cut(z[:, :2].astype(np.int64), z[:, 2].astype(np.float32), n + 5, missing_distance(t))
        assert np.array_equal(got, want), (n, t)
        assert 1 < len(np.unique(want)) < n + 5
        rep, _ = engine.cluster_greedy(rows, n + 5, t)
        assert np.array_equal(want[rep], want)                         # a genome and its representative share a component


def test_tree_single_api_cpu_build(emu_engine):
    argument_errors(emu_engine)
    small_inputs(emu_engine, 1)


def test_tree_single_scipy_cpu_build(emu_engine):
    matches_scipy(emu_engine, 6)


def test_tree_single_properties_cpu_build(emu_engine):
    properties(emu_engine, 7, ((60, 90, 95.0), (300, 500, 95.0), (300, 2000, 80.0), (1000, 1500, 97.0)))


def species_rows(rng, n, per_species=50):
    """species blocks of `per_species` consecutive genomes: a random spanning structure inside each block plus extra pairs, both directions
    of a pair, identities 95 - 100 inside; a few pairs between species at 78 - 95"""
    base = np.arange(n) // per_species * per_species
    inside = [(np.arange(n), base + rng.integers(0, per_species, n)) for _ in range(2)]
    a = np.concatenate([x for x, _ in inside] + [rng.integers(0, n, n // 20)])
    b = np.concatenate([np.minimum(y, n - 1) for _, y in inside] + [rng.integers(0, n, n // 20)])
    x = np.where(a // per_species == b // per_species, 95 + 5 * rng.random(len(a)), 78 + 17 * rng.random(len(a))).astype(np.float32)
    both = rng.random(len(a)) < 0.5
    rows = np.zeros(len(a) + int(both.sum()), dtype=CGI_DT)
    rows["qryGenomeId"] = np.concatenate([a, b[both]])
    rows["refGenomeId"] = np.concatenate([b, a[both]])
    rows["identity"] = np.concatenate([x, (x[both] - np.float32(0.01)).astype(np.float32)])
    return rows[rng.permutation(len(rows))]


@pytest.mark.gpu
def test_tree_single_api_gpu(gpu_engine):
    argument_errors(gpu_engine)
    small_inputs(gpu_engine, 2)
    matches_scipy(gpu_engine, 8)
    rng = np.random.default_rng(3)
    for n, pairs in ((1000, 20000), (2500, 60000)):
        check(gpu_engine, random_identity_rows(rng, n, pairs), n)
        check(gpu_engine, random_identity_rows(rng, n, pairs, integer=True), n, 75.0)
        check(gpu_engine, random_rows(rng, n, pairs, 95.0), n)
    check(gpu_engine, make_rows([]), 700)
    check(gpu_engine, clique_rows(rng, 600, 95.0), 600)
    check(gpu_engine, path_rows(2000, 95.0), 2000)
    check(gpu_engine, hub_rows(1500), 1500)
    properties(gpu_engine, 9, ((1000, 3000, 95.0), (2500, 20000, 80.0), (2500, 4000, 97.0)))


@pytest.mark.gpu
def test_tree_single_beyond_the_dense_ceiling_gpu(gpu_engine):
    """More genomes than any dense method takes: 150 000 (a float matrix of 90 GB), or as many more as it takes for that matrix to exceed
    the device's free memory, so that a result proves the call never held one."""
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert gpu_engine.lib.ani_device_memory(gpu_engine.h, ctypes.byref(free), ctypes.byref(total)) == 0
    n = 150000
    if 4 * n * n <= free.value:
        n = (int(math.sqrt(free.value / 4.0)) // 50 + 2) * 50
    print("free device memory %.1f GB, %d genomes, dense matrix %.1f GB" % (free.value / 1e9, n, 4.0 * n * n / 1e9))
    assert free.value < 4 * n * n
    rows = species_rows(np.random.default_rng(11), n)
    assert 2 * 10 ** 5 <= len(rows) <= 10 ** 6
    z, _ = check(gpu_engine, rows, n)
    assert 0 < (z[:, 2] < 1.0).sum() < n - 1
    print("%d rows, %d forest edges, %d rounds" % (len(rows), int((z[:, 2] < 1.0).sum()), gpu_engine.tree_single_rounds()))


@pytest.mark.gpu
def test_tree_single_rows_of_the_engine_gpu(gpu_engine):
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
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def clade_lengths(children, height, names):
    """-> {clade: branch length above it} with a node at half its merge distance above its leaves, root clade"""
    clade = [frozenset([x]) for x in names]
    h = [0.0] * len(names)
    lengths = {}
    for s, (x, y) in enumerate(children.tolist()):
        for c in (x, y):
            lengths[clade[c]] = (float(height[s]) - h[c]) / 2
        clade.append(clade[x] | clade[y])
        h.append(float(height[s]))
    return lengths, clade[-1]


def single_from_matrix(path):
    """the restatement over the printed .matrix values -> {clade: branch length}, root clade, the .mst text"""
    names, cells = read_matrix(path)
    n = len(names)
    keys = sorted(cells)
    rows = make_rows([(j, i, np.float32(cells[(j, i)])) for j, i in keys])
    children, height, edges = expected(rows, n, 0.0)
    lengths, top = clade_lengths(children, height, names)
    mst = "".join("%s\t%s\t%s\tani\n" % (names[a], names[b], cells[(a, b)]) for (a, b), d in zip(edges.tolist(), height.tolist()) if d < 1.0)
    return lengths, top, mst, height


def run_cli(binary, tmp, n_len, variants=()):
    lst = tree_genomes(tmp, n_len)
    base = os.path.join(tmp, "plain.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "-o", base], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    # without the option: no .mst, and the other files as they were
    upgma = os.path.join(tmp, "u.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "-o", upgma], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert not os.path.exists(base + ".mst") and not os.path.exists(upgma + ".mst")
    assert open(upgma, "rb").read() == open(base, "rb").read() and open(upgma + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    out = os.path.join(tmp, "t.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "--treeMethod", "single", "-o", out], capture_output=True,
                       env=dict(os.environ, ANI_CLI_TRACE="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"tree written" in r.stderr and b"spanning tree written" in r.stderr
    assert open(out, "rb").read() == open(base, "rb").read()                           # -o and .matrix unchanged
    assert open(out + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    text = open(out + ".newick").read()
    want, want_root, want_mst, height = single_from_matrix(base + ".matrix")
    got, root = parse_newick(text)
    assert root == want_root and set(got) == set(want)
    for c in want:
        assert abs(got[c] - want[c]) <= 1e-6, (sorted(c), got[c], want[c])
    assert text != open(upgma + ".newick").read()                                      # not the average-linkage tree
    # .mst: n - components lines, each a .matrix cell with its value, in ascending distance
    names, cells = read_matrix(base + ".matrix")
    mst = open(out + ".mst").read()
    lines = [ln.split("\t") for ln in mst.splitlines()]
    components = int((height >= 1.0).sum()) + 1
    assert components == 2 and len(lines) == len(names) - components
    for a, b, v, source in lines:
        assert names.index(a) < names.index(b) and cells[(names.index(a), names.index(b))] == v and source == "ani"
    vals = [float(ln[2]) for ln in lines]
    assert vals == sorted(vals, reverse=True)
    assert mst == want_mst
    # the same files through the other paths of the command line
    for name, args in variants:
        o = os.path.join(tmp, "v_%s.out" % name)
        r = subprocess.run([binary] + [a.replace("@L", lst).replace("@T", tmp) for a in args] + ["--tree", "--treeMethod", "single", "-o", o],
                           capture_output=True)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert open(o + ".newick").read() == text and open(o + ".mst").read() == mst, name
    # other values are refused, and the refusal names all three methods; the method needs --tree
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--tree", "--treeMethod", "bogus", "-o", os.path.join(tmp, "bad.out")], capture_output=True)
    assert r.returncode == 1 and b"ERROR, --treeMethod takes average or nj or single" in r.stderr
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--treeMethod", "single", "-o", os.path.join(tmp, "bad.out")], capture_output=True)
    assert r.returncode == 1 and b"--treeMethod needs --tree" in r.stderr
    return text


def run_cli_single_genome(binary, tmp):
    p = os.path.join(tmp, "one genome.fa")
    orc.write_fasta(p, [orc.synth_genome(17, 0, 30000)], names=["x"])
    out = os.path.join(tmp, "one.out")
    r = subprocess.run([binary, "-q", p, "-r", p, "--tree", "--treeMethod", "single", "-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out + ".newick").read() == "'%s';\n" % p
    assert open(out + ".mst").read() == ""


def run_cli_fill(binary, engine, tmp, n_len):
    """--treeFill sketch across two genera that the mapping cannot relate but whose sketches share values: the spanning tree crosses on a
    sketch estimate"""
    import fastani_amd
    from test_sigdist import two_genera
    size = 2000
    lst, paths, genomes = two_genera(tmp, n_len)
    base, out = os.path.join(tmp, "b.out"), os.path.join(tmp, "f.out")
    for extra, o in (([], base), (["--treeFill", "sketch", "--sketchSize", str(size)], out)):
        r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "--treeMethod", "single"] + extra + ["-o", o], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    names, cells = read_matrix(base + ".matrix")
    assert names == paths
    plain = [ln.split("\t") for ln in open(base + ".mst").read().splitlines()]
    assert len(plain) == 4 and all(ln[3] == "ani" for ln in plain)                      # two genera of three: two components
    # the same through the API: the printed cells, then the fill rows
    sk = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes)
    sig, length = sk.signatures(size)
    sk.close()
    pairs = engine.signature_pairs(sig, length, 16, 1)
    fill = [(int(r["a"]), int(r["b"]), r["identity"]) for r in pairs if (int(r["a"]), int(r["b"])) not in cells and r["identity"] > 0]
    assert fill and all(a < 3 <= b for a, b, _ in fill)
    rows = make_rows([(j, i, np.float32(cells[(j, i)])) for j, i in sorted(cells)] + fill)
    children, height, edges = expected(rows, len(names), 0.0)
    est = {(a, b): w for a, b, w in fill}
    want = ""
    for (a, b), d in zip(edges.tolist(), height.tolist()):
        assert d < 1.0
        want += "%s\t%s\t%s\t%s\n" % (names[a], names[b], cells[(a, b)] if (a, b) in cells else "%f" % est[(a, b)], "ani" if (a, b) in cells else "sketch")
    got = open(out + ".mst").read()
    assert got == want
    assert [ln.split("\t")[3] for ln in got.splitlines()] == ["ani"] * 4 + ["sketch"]
    got_l, root = parse_newick(open(out + ".newick").read())
    want_l, want_root = clade_lengths(children, height, names)
    assert root == want_root == frozenset(names) and set(got_l) == set(want_l)
    for c in want_l:
        assert abs(got_l[c] - want_l[c]) <= 1e-6, (sorted(c), got_l[c], want_l[c])


def test_cli_tree_single_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 30000, VARIANTS)


def test_cli_tree_single_one_genome_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli_single_genome(os.path.join(EMU, "fastANI_emu"), str(tmp_path))


def test_cli_tree_single_fill_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli_fill(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 50000)


@pytest.mark.gpu
def test_cli_tree_single_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    for sub in ("a", "b", "c"):
        os.mkdir(os.path.join(str(tmp_path), sub))
    run_cli(binary, os.path.join(str(tmp_path), "a"), 200000, VARIANTS)
    run_cli_single_genome(binary, os.path.join(str(tmp_path), "b"))
    run_cli_fill(binary, gpu_engine, os.path.join(str(tmp_path), "c"), 200000)
