"""Average-linkage (UPGMA) tree (ani_tree_average, Engine.tree_average, fastANI --tree) against a plain-Python statement of its
semantics.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import orc
from fastani_amd.api import CGI_DT, AniError
from test_cluster import VARIANTS, clique_rows, make_rows, pair_weights, path_rows, random_rows, read_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the semantics, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def leaf_matrix(n, lo, hi, w, missing):
    """rules 1-2: float32 distances, d = (float)(1 - (double)w / 100), a pair without rows at the missing identity; +inf on the diagonal"""
    d = np.full((n, n), np.float32(1.0 - np.float64(missing) / 100.0), dtype=np.float32)
    x = (1.0 - w.astype(np.float64) / 100.0).astype(np.float32)
    d[lo, hi] = x
    d[hi, lo] = x
    np.fill_diagonal(d, np.inf)
    return d


def average(dak, dbk, na, nb):
    """rule 4's update, in double, rounded to float once"""
    return ((na * dak.astype(np.float64) + nb * dbk.astype(np.float64)) / np.float64(na + nb)).astype(np.float32)


def upgma_simple(d):
    """rules 3-5 with the full argmin at every step (n <= ~300): -> children (n - 1, 2) int64, heights float32"""
    n = len(d)
    d = d.copy()
    size = np.ones(n, dtype=np.int64)
    ids = np.arange(n)
    active = np.ones(n, dtype=bool)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    children = np.zeros((max(n - 1, 0), 2), dtype=np.int64)
    height = np.zeros(max(n - 1, 0), dtype=np.float32)
    for s in range(n - 1):
        v = np.where(upper & active[:, None] & active[None, :], d, np.float32(np.inf))
        a, b = divmod(int(np.flatnonzero(v == v.min())[0]), n)      # row-major: the smallest a, then the smallest b
        children[s] = sorted((ids[a], ids[b]))
        height[s] = d[a, b]
        k = active.copy()
        k[[a, b]] = False
        new = average(d[a, k], d[b, k], size[a], size[b])
        d[a, k] = new
        d[k, a] = new
        active[b] = False
        size[a] += size[b]
        ids[a] = n + s
    return children, height


def upgma_rowmin(d):
    """the same with a cached (d, column) minimum per row, rescanned only when rule 4 can have raised it (larger n)"""
    n = len(d)
    d = d.copy()
    size = np.ones(n, dtype=np.int64)
    ids = np.arange(n)
    active = np.ones(n, dtype=bool)
    children = np.zeros((max(n - 1, 0), 2), dtype=np.int64)
    height = np.zeros(max(n - 1, 0), dtype=np.float32)
    if n < 2:
        return children, height
    rm, rc = d.min(axis=1), d.argmin(axis=1)                        # argmin: the first, i.e. smallest, column of the minimum
    for s in range(n - 1):
        act = np.flatnonzero(active)
        lo, hi = np.minimum(act, rc[act]), np.maximum(act, rc[act])
        key = (rm[act].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (lo.astype(np.uint64) << np.uint64(16)) | hi.astype(np.uint64)
        i = int(np.argmin(key))
        a, b = int(lo[i]), int(hi[i])
        children[s] = sorted((ids[a], ids[b]))
        height[s] = d[a, b]
        k = active.copy()
        k[[a, b]] = False
        kk = np.flatnonzero(k)
        new = average(d[a, kk], d[b, kk], size[a], size[b])
        d[a, kk] = new
        d[kk, a] = new
        d[:, b] = np.inf
        d[b, :] = np.inf
        active[b] = False
        size[a] += size[b]
        ids[a] = n + s
        m, c = rm[kk], rc[kk]
        rescan = ((c == a) | (c == b)) & (new > m)
        better = ~rescan & ((new < m) | ((new == m) & (a < c)))
        rm[kk[better]], rc[kk[better]] = new[better], a
        for r in kk[rescan].tolist() + [a]:
            rm[r], rc[r] = d[r].min(), d[r].argmin()
    return children, height


def expected(rows, n, missing, simple=None):
    d = leaf_matrix(n, *pair_weights(rows), missing)
    if simple is None:
        simple = n <= 300
    return (upgma_simple if simple else upgma_rowmin)(d)


def hub_rows(n, spoke=99.0, rim=80.0):
    """genome 0 close to every other; the others far from each other, their pairs in order: after the first merge every row's minimum
    sits in slot 0 and rises, so every merge rescans every row"""
    pairs = [(0, i, spoke) for i in range(1, n)]
    pairs += [(i, i + 1, rim) for i in range(1, n - 1)]
    return make_rows(pairs)


def check(engine, rows, n, missing=0.0):
    z = engine.tree_average(rows, n, missing)
    children, height = expected(rows, n, missing)
    m = max(n - 1, 0)
    assert z.dtype == np.float64 and z.shape == (m, 4)
    got_c = z[:, :2].astype(np.int64)
    got_h = z[:, 2].astype(np.float32)
    assert np.array_equal(got_h.astype(np.float64), z[:, 2])         # float32 heights, exact in float64
    bad = np.nonzero((got_c != children).any(axis=1) | (got_h.view(np.uint32) != height.view(np.uint32)))[0]
    assert len(bad) == 0, (bad[:5], got_c[bad[:5]], children[bad[:5]], got_h[bad[:5]], height[bad[:5]])
    assert (np.diff(got_h) >= 0).all()
    if m:
        count = np.ones(n + m)
        for s in range(m):
            count[n + s] = count[children[s, 0]] + count[children[s, 1]]
        assert np.array_equal(z[:, 3], count[n:])
        hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
        assert hierarchy.is_valid_linkage(z)
    return z


def random_identity_rows(rng, n, n_pairs, integer=False):
    a = rng.integers(0, n, n_pairs)
    b = rng.integers(0, n, n_pairs)
    x = rng.integers(76, 101, n_pairs).astype(np.float32) if integer else (76 + 24 * rng.random(n_pairs)).astype(np.float32)
    rows = np.zeros(n_pairs, dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"], rows["identity"] = a, b, np.maximum(x, np.float32(0.5))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against itself
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatements_agree():
    rng = np.random.default_rng(5)
    cases = [(random_identity_rows(rng, 60, 400), 60, 0.0), (random_identity_rows(rng, 80, 300, integer=True), 80, 0.0),
             (random_identity_rows(rng, 50, 900, integer=True), 50, 75.0), (random_rows(rng, 70, 500, 95.0), 75, 0.0),
             (make_rows([]), 20, 0.0), (make_rows([]), 20, 50.0), (clique_rows(rng, 40, 95.0), 40, 0.0), (path_rows(60, 95.0), 60, 0.0),
             (hub_rows(40), 40, 0.0), (hub_rows(40), 40, 85.0)]
    for rows, n, missing in cases:
        d = leaf_matrix(n, *pair_weights(rows), missing)
        c1, h1 = upgma_simple(d)
        c2, h2 = upgma_rowmin(d)
        assert np.array_equal(c1, c2) and np.array_equal(h1.view(np.uint32), h2.view(np.uint32)), n
        assert (np.diff(h1) >= 0).all()


def test_restatement_matches_scipy():
    """tie-free random distances: scipy's average linkage merges the same leaf sets; heights to a relative 1e-5 (scipy stays in double)"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(6)
    n = 120
    a, b = np.triu_indices(n, 1)
    rows = np.zeros(len(a), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = a, b
    rows["identity"] = (70 + 30 * rng.random(len(a))).astype(np.float32)
    rows["identity"] = np.maximum(rows["identity"], np.float32(70.001))
    d = leaf_matrix(n, *pair_weights(rows), 0.0)
    children, height = upgma_simple(d)
    dd = d.astype(np.float64)
    np.fill_diagonal(dd, 0.0)
    z = hierarchy.linkage(dd[a, b], method="average")

    def leafsets(ch):
        sets = [frozenset([i]) for i in range(n)]
        for x, y in ch:
            sets.append(sets[int(x)] | sets[int(y)])
        return sets[n:]
    assert leafsets(children) == leafsets(z[:, :2].astype(np.int64))
    assert np.allclose(height.astype(np.float64), z[:, 2], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    rows = make_rows([(0, 1, 97.0), (1, 2, 96.0)])
    for missing in (-1.0, 100.5, float("nan")):
        with pytest.raises(AniError) as ex:
            engine.tree_average(rows, 3, missing)
        assert ex.value.code == -1, missing                            # ANI_ERR_ARG
    for bad in ((0, 3, 97.0), (-1, 1, 97.0), (2, 5, 97.0), (0, 2, 0.0), (0, 2, -3.0), (0, 2, 100.5), (1, 1, float("nan")), (0, 1, float("inf"))):
        with pytest.raises(AniError) as ex:
            engine.tree_average(make_rows([(0, 1, 97.0), bad]), 3)
        assert ex.value.code == -1, bad
    with pytest.raises(AniError) as ex:
        engine.tree_average(rows, -1)
    assert ex.value.code == -1
    ch, h = np.zeros(4, np.int32), np.zeros(2, np.float32)
    assert engine.lib.ani_tree_average(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), None, h.ctypes.data) == -1
    assert engine.lib.ani_tree_average(engine.h, rows.ctypes.data, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, None) == -1
    assert engine.lib.ani_tree_average(engine.h, None, 2, 3, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data) == -1
    # limits, before anything is allocated or read: 65 537 genomes, 2^32 rows
    assert engine.lib.ani_tree_average(engine.h, rows.ctypes.data, 2, 65537, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data) == -4
    assert engine.lib.ani_tree_average(engine.h, rows.ctypes.data, 1 << 32, 3, ctypes.c_float(0.0), ch.ctypes.data, h.ctypes.data) == -4
    # n <= 1: nothing to merge, nothing written
    for n in (0, 1):
        assert engine.tree_average(make_rows([]), n).shape == (0, 4)
    assert engine.tree_average(make_rows([(0, 0, 100.0)]), 1).shape == (0, 4)
    assert engine.lib.ani_tree_average(engine.h, None, 0, 1, ctypes.c_float(0.0), None, None) == 0
    # missing identity 0 and 100 are both allowed
    check(engine, rows, 3, 100.0)


def small_inputs(engine, seed):
    rng = np.random.default_rng(seed)
    # n = 2 with and without rows; no rows at all (every distance 1: ties everywhere)
    z = check(engine, make_rows([]), 2)
    assert z.tolist() == [[0.0, 1.0, 1.0, 2.0]]
    check(engine, make_rows([(1, 0, 97.5)]), 2)
    check(engine, make_rows([]), 9)
    check(engine, make_rows([]), 9, 75.0)
    # fold order: the result depends on the order given; self rows ignored
    rows = make_rows([(1, 0, 94.0), (0, 1, 96.5), (1, 0, 95.25), (2, 3, 95.0), (3, 2, 94.999), (4, 4, 100.0), (0, 2, 90.0)])
    check(engine, rows, 7)
    check(engine, rows[::-1].copy(), 7)
    check(engine, rows, 7, 75.0)
    for n, pairs in ((12, 40), (70, 500), (130, 700)):
        check(engine, random_identity_rows(rng, n, pairs), n)
        check(engine, random_identity_rows(rng, n, pairs), n, 75.0)
        check(engine, random_identity_rows(rng, n, pairs, integer=True), n)       # integer identities: many equal distances
        check(engine, random_rows(rng, n, pairs, 95.0), n + 3)                    # several rows per pair in both orders, self rows
    check(engine, clique_rows(rng, 70, 95.0), 70)
    check(engine, path_rows(100, 95.0), 100)
    check(engine, hub_rows(90), 90)
    check(engine, hub_rows(90), 90, 85.0)


def test_tree_api_cpu_build(emu_engine):
    argument_errors(emu_engine)
    small_inputs(emu_engine, 1)


@pytest.mark.gpu
def test_tree_api_gpu(gpu_engine):
    argument_errors(gpu_engine)
    small_inputs(gpu_engine, 2)
    rng = np.random.default_rng(3)
    for n, pairs in ((1000, 20000), (2500, 60000)):
        check(gpu_engine, random_identity_rows(rng, n, pairs), n)
        check(gpu_engine, random_identity_rows(rng, n, pairs, integer=True), n, 75.0)
        check(gpu_engine, random_rows(rng, n, pairs, 95.0), n)
    check(gpu_engine, make_rows([]), 700)
    check(gpu_engine, clique_rows(rng, 600, 95.0), 600)
    check(gpu_engine, path_rows(2000, 95.0), 2000)
    check(gpu_engine, hub_rows(1500), 1500)


@pytest.mark.gpu
def test_tree_rows_of_the_engine_gpu(gpu_engine):
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
def read_name(s, i):
    if s[i] != "'":
        j = i
        while s[j] not in "(),:;":
            j += 1
        return s[i:j], j
    out, j = [], i + 1
    while True:
        if s[j] == "'" and s[j + 1:j + 2] == "'":
            out.append("'")
            j += 2
        elif s[j] == "'":
            return "".join(out), j + 1
        else:
            out.append(s[j])
            j += 1


def parse_newick(text):
    """-> {clade (frozenset of leaf names): branch length above it}, root clade"""
    assert text.endswith(";\n")
    s = text[:-2]
    lengths, stack, last, i = {}, [[]], None, 0
    while i < len(s):
        c = s[i]
        if c == "(":
            stack.append([])
            i += 1
        elif c == ",":
            i += 1
        elif c == ")":
            kids = stack.pop()
            assert len(kids) == 2
            last = frozenset().union(*kids)
            stack[-1].append(last)
            i += 1
        elif c == ":":
            j = i + 1
            while j < len(s) and s[j] not in ",)":
                j += 1
            lengths[last] = float(s[i + 1:j])
            i = j
        else:
            name, i = read_name(s, i)
            last = frozenset([name])
            stack[-1].append(last)
    assert len(stack) == 1 and len(stack[0]) == 1
    return lengths, stack[0][0]


def tree_from_matrix(path):
    """the restatement over the printed .matrix values -> {clade: branch length}, root clade, merge heights"""
    names, cells = read_matrix(path)
    n = len(names)
    keys = sorted(cells)
    rows = make_rows([(j, i, np.float32(cells[(j, i)])) for j, i in keys])
    children, height = expected(rows, n, 0.0)
    clade = [frozenset([x]) for x in names]
    h = [0.0] * n
    lengths = {}
    for s, (x, y) in enumerate(children.tolist()):
        for c in (x, y):
            lengths[clade[c]] = (float(height[s]) - h[c]) / 2
        clade.append(clade[x] | clade[y])
        h.append(float(height[s]))
    return lengths, clade[-1], height


def tree_genomes(tmp, n_len):
    """two species (six and three related genomes, no ANI between them): one merge at distance 1, the others well apart; two of the
    file names need quoting"""
    paths = []
    for i, g in enumerate(list(range(0, 6)) + [20, 21, 22]):
        name = {1: "it's (a) genome,1.fa", 7: "g 7;x:[y].fa"}.get(i, "t%d.fa" % i)
        p = os.path.join(tmp, name)
        orc.write_fasta(p, [orc.synth_genome(17, g, n_len)], names=["t%d" % i])
        paths.append(p)
    lst = os.path.join(tmp, "l.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst


def run_cli(binary, tmp, n_len, variants=()):
    lst = tree_genomes(tmp, n_len)
    base = os.path.join(tmp, "plain.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "-o", base], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert not os.path.exists(base + ".newick")
    out = os.path.join(tmp, "t.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--tree", "-o", out], capture_output=True, env=dict(os.environ, ANI_CLI_TRACE="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"tree written" in r.stderr
    assert open(out, "rb").read() == open(base, "rb").read()                           # -o and .matrix unchanged
    assert open(out + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    text = open(out + ".newick").read()
    quoted = [x for x in open(lst).read().split("\n") if x.endswith((",1.fa", "[y].fa"))]
    assert len(quoted) == 2
    for x in quoted:
        assert "'%s':" % x.replace("'", "''") in text
    want, want_root, height = tree_from_matrix(base + ".matrix")
    assert (np.diff(height.astype(np.float64)) > 1e-5).all(), height                 # merges well apart: the printed values decide alike
    got, root = parse_newick(text)
    assert root == want_root and set(got) == set(want)
    for c in want:
        assert abs(got[c] - want[c]) <= 1e-6, (sorted(c), got[c], want[c])
    # the same tree through the other paths of the command line
    for name, args in variants:
        o = os.path.join(tmp, "v_%s.out" % name)
        r = subprocess.run([binary] + [a.replace("@L", lst).replace("@T", tmp) for a in args] + ["--tree", "-o", o], capture_output=True)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert open(o + ".newick").read() == text, name
    return text


def test_cli_tree_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 30000, VARIANTS)


def test_cli_tree_single_genome_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    p = os.path.join(str(tmp_path), "one genome.fa")
    orc.write_fasta(p, [orc.synth_genome(17, 0, 30000)], names=["x"])
    out = os.path.join(str(tmp_path), "one.out")
    r = subprocess.run([os.path.join(EMU, "fastANI_emu"), "-q", p, "-r", p, "--tree", "-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out + ".newick").read() == "'%s';\n" % p


@pytest.mark.gpu
def test_cli_tree_gpu(tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, str(tmp_path), 200000, VARIANTS)
