"""Greedy species clustering (ani_cluster_greedy, Engine.cluster_greedy, fastANI --cluster) against a plain-Python statement of its
semantics.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import orc
from fastani_amd.api import CGI_DT, AniError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the semantics, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_weights(rows):
    """-> (lo, hi, w) per pair: the rows of a pair folded in the order given (the first sets w, every later one w = (w + id) / 2 in
    float32), self rows skipped"""
    q = rows["qryGenomeId"].astype(np.int64)
    r = rows["refGenomeId"].astype(np.int64)
    x = rows["identity"].astype(np.float32)
    keep = q != r
    lo, hi, x = np.minimum(q, r)[keep], np.maximum(q, r)[keep], x[keep]
    order = np.argsort(lo * (1 << 32) + hi, kind="stable")
    lo, hi, x = lo[order], hi[order], x[order]
    if len(x) == 0:
        return lo, hi, x
    head = np.ones(len(x), dtype=bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    first = np.nonzero(head)[0]
    size = np.diff(np.append(first, len(x)))
    w = x[first].copy()
    for k in range(1, int(size.max())):                           # the k-th row of every pair that has one, all pairs at once
        m = size > k
        w[m] = (w[m] + x[first[m] + k]) / np.float32(2)
    return lo[first], hi[first], w


def greedy(n, lo, hi, w, t):
    """representatives in index order; a member goes to the adjacent representative with the largest w (ties: smallest id)"""
    e = w >= np.float32(t)
    lo, hi, w = lo[e].tolist(), hi[e].tolist(), w[e]
    lower = [[] for _ in range(n)]
    adj = [[] for _ in range(n)]
    for a, b, x in zip(lo, hi, w.tolist()):
        lower[b].append(a)
        adj[a].append((b, x))
        adj[b].append((a, x))
    is_rep = [False] * n
    for i in range(n):
        is_rep[i] = not any(is_rep[j] for j in lower[i])
    rep = np.arange(n, dtype=np.int32)
    ident = np.zeros(n, dtype=np.float32)
    for i in range(n):
        if is_rep[i]:
            continue
        best = None
        for j, x in adj[i]:                                         # (x: the float32 value as a Python float, exact)
            if is_rep[j] and (best is None or x > best[1] or (x == best[1] and j < best[0])):
                best = (j, x)
        rep[i], ident[i] = best
    return rep, ident


def make_rows(pairs):
    """pairs: list of (q, r, identity) -> CGI_DT array in that order"""
    a = np.zeros(len(pairs), dtype=CGI_DT)
    if pairs:
        q, r, x = zip(*pairs)
        a["qryGenomeId"], a["refGenomeId"], a["identity"] = q, r, np.asarray(x, dtype=np.float32)
    return a


def random_rows(rng, n_genomes, n_pairs, t):
    """pairs with both directions, one direction and three or more rows, identities on a grid that holds t exactly, self rows"""
    grid = np.float32(t) + np.arange(-8, 9, dtype=np.float32) * np.float32(0.25)
    a = rng.integers(0, n_genomes, n_pairs)
    b = rng.integers(0, n_genomes, n_pairs)
    reps = rng.choice([1, 1, 2, 2, 3, 4], n_pairs)
    q = np.repeat(a, reps)
    r = np.repeat(b, reps)
    flip = rng.random(len(q)) < 0.5                                # both directions, in either order
    q, r = np.where(flip, r, q), np.where(flip, q, r)
    x = grid[rng.integers(0, len(grid), len(q))]
    x[rng.random(len(q)) < 0.1] = np.float32(t)                    # weights exactly at the threshold
    rows = np.zeros(len(q), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"], rows["identity"] = q, r, x
    rows = rows[rng.permutation(len(rows))]                        # the fold follows the order given, whatever it is
    selfs = np.zeros(max(1, len(rows) // 50), dtype=CGI_DT)
    g = rng.integers(0, n_genomes, len(selfs))
    selfs["qryGenomeId"], selfs["refGenomeId"], selfs["identity"] = g, g, np.float32(100)
    return np.concatenate([rows, selfs])[rng.permutation(len(rows) + len(selfs))]


def clique_rows(rng, m, t, base=0):
    a, b = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    keep = a != b
    rows = np.zeros(int(keep.sum()), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = base + a[keep], base + b[keep]
    rows["identity"] = np.float32(t) + rng.integers(0, 40, len(rows)).astype(np.float32) * np.float32(0.125)
    return rows


def path_rows(m, t):
    return make_rows([(i + 1, i, np.float32(t) + np.float32(i % 7) * np.float32(0.5)) for i in range(m - 1)])


def check(engine, rows, n, t):
    rep, ident = engine.cluster_greedy(rows, n, t)
    erep, eident = greedy(n, *pair_weights(rows), t)
    assert rep.dtype == np.int32 and ident.dtype == np.float32 and len(rep) == n
    bad = np.nonzero((rep != erep) | (ident.view(np.uint32) != eident.view(np.uint32)))[0]
    assert len(bad) == 0, (bad[:10], rep[bad[:10]], erep[bad[:10]], ident[bad[:10]], eident[bad[:10]])
    return rep


def argument_errors(engine):
    rows = make_rows([(0, 1, 97.0), (1, 2, 96.0)])
    for t in (0.0, -1.0, 100.5, float("nan")):
        with pytest.raises(AniError) as ex:
            engine.cluster_greedy(rows, 3, t)
        assert ex.value.code == -1, t                            # ANI_ERR_ARG
    for bad in ((0, 3, 97.0), (-1, 1, 97.0), (2, 5, 97.0)):
        with pytest.raises(AniError) as ex:
            engine.cluster_greedy(make_rows([(0, 1, 97.0), bad]), 3, 95.0)
        assert ex.value.code == -1, bad
    with pytest.raises(AniError) as ex:
        engine.cluster_greedy(rows, 1, 95.0)
    assert ex.value.code == -1
    # 2^32 rows: ANI_ERR_LIMIT before a row is read
    rep, ident = np.zeros(3, np.int32), np.zeros(3, np.float32)
    rc = engine.lib.ani_cluster_greedy(engine.h, rows.ctypes.data, 1 << 32, 3, ctypes.c_float(95.0), rep.ctypes.data, ident.ctypes.data)
    assert rc == -4
    # no rows, and T = 100 allowed
    rep, ident = engine.cluster_greedy(make_rows([]), 5, 95.0)
    assert rep.tolist() == list(range(5)) and not ident.any()
    rep, ident = engine.cluster_greedy(make_rows([(0, 1, 100.0), (2, 1, 99.0)]), 3, 100.0)
    assert rep.tolist() == [0, 0, 2] and ident.tolist() == [0.0, 100.0, 0.0]


def small_graphs(engine, seed):
    rng = np.random.default_rng(seed)
    # fold order: (a, b) then (b, a) then (a, b) again — the result depends on the order given
    rows = make_rows([(1, 0, 94.0), (0, 1, 96.5), (1, 0, 95.25), (2, 3, 95.0), (3, 2, 94.999), (4, 4, 100.0)])
    rep = check(engine, rows, 7, 95.0)
    assert rep.tolist() == [0, 0, 2, 3, 4, 5, 6]                  # (2, 3) averages below T; 4 self only; 5, 6 isolated
    # a member of a later representative (r > i): 0 - 1 - 2 with {0, 1} and {1, 2} edges, 1 joins 0; then 3 - 1 ... 3 is its own
    rows = make_rows([(0, 2, 99.0), (1, 2, 97.0), (3, 1, 98.0), (3, 4, 99.5)])
    check(engine, rows, 5, 95.0)
    # ties: equal weights to two representatives -> the smaller id
    rows = make_rows([(0, 2, 97.0), (1, 2, 97.0)])
    assert check(engine, rows, 3, 95.0).tolist() == [0, 1, 0]
    for n, pairs in ((30, 60), (200, 900), (1000, 3000), (400, 20000)):
        for t in (95.0, 80.0, 99.0):
            check(engine, random_rows(rng, n, pairs, t), n + 7, t)   # + 7 genomes without rows
    # a clique (long lower lists: the wave-wide scans) beside random rows, and an ordered path (one decision per round)
    rows = np.concatenate([clique_rows(rng, 300, 95.0, base=50), random_rows(rng, 600, 2000, 95.0)])
    check(engine, rows, 600, 95.0)
    rep = check(engine, path_rows(3000, 95.0), 3000, 95.0)
    assert rep[::2].tolist() == list(range(0, 3000, 2))


def test_cluster_api_cpu_build(emu_engine):
    argument_errors(emu_engine)
    small_graphs(emu_engine, 1)


@pytest.mark.gpu
def test_cluster_api_gpu(gpu_engine):
    argument_errors(gpu_engine)
    small_graphs(gpu_engine, 2)
    rng = np.random.default_rng(3)
    for n, pairs, t in ((20000, 480000, 95.0), (3000, 480000, 95.0), (100000, 500000, 80.0)):
        rows = random_rows(rng, n, pairs, t)
        assert len(rows) >= 10 ** 6
        check(gpu_engine, rows, n, t)
    check(gpu_engine, clique_rows(rng, 3000, 95.0), 3000, 95.0)         # 9 * 10^6 rows
    rep = check(gpu_engine, path_rows(100000, 95.0), 100000, 95.0)
    assert rep[::2].tolist() == list(range(0, 100000, 2))


@pytest.mark.gpu
def test_cluster_rows_of_the_engine_gpu(gpu_engine):
    """rows from the mapping path itself (Sketch.map_cgi_batch over synthetic species clusters), clustered at several thresholds"""
    import fastani_amd
    e = gpu_engine
    p = e.params(16, 3000)
    genomes = [[orc.synth_genome(13, g, 120000)] for g in list(range(0, 12)) + list(range(20, 30)) + [40, 41, 60]]
    sk = fastani_amd.Sketch(e, p, genomes)
    rows = sk.map_cgi_batch(genomes, 0)
    assert len(rows) > 100
    ids = np.unique(rows["identity"][rows["qryGenomeId"] != rows["refGenomeId"]])
    for t in np.quantile(ids, [0.1, 0.5, 0.9]).tolist() + [95.0]:
        check(e, rows, len(genomes), t)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def read_matrix(path):
    """-> names, {(i, j): (value string, float32)} for i > j"""
    lines = open(path).read().splitlines()
    n = int(lines[0])
    names, cells = [], {}
    for i in range(n):
        f = lines[1 + i].split("\t")
        names.append(f[0])
        for j, v in enumerate(f[1:]):
            if v != "NA":
                cells[(j, i)] = v
    return names, cells


def clusters_from_matrix(path, t):
    names, cells = read_matrix(path)
    keys = sorted(cells)
    lo = np.array([k[0] for k in keys], dtype=np.int64)
    hi = np.array([k[1] for k in keys], dtype=np.int64)
    rep, _ = greedy(len(names), lo, hi, np.array([float(cells[k]) for k in keys], dtype=np.float32), t)
    out = []
    for i in range(len(names)):
        j = int(rep[i])
        out.append("%s\t%s\t%s" % (names[i], names[j], "NA" if i == j else cells[(min(i, j), max(i, j))]))
    return "\n".join(out) + "\n"


def thresholds(path, k=3):
    """k thresholds inside the range of the printed values, each at least 1e-5 away from every printed value"""
    _, cells = read_matrix(path)
    vals = sorted({float(v) for v in cells.values()})
    gaps = [(a + b) / 2 for a, b in zip(vals, vals[1:]) if b - a > 2e-5]
    assert len(gaps) >= k, vals
    return [gaps[int(i)] for i in np.linspace(0, len(gaps) - 1, k)]


def cluster_genomes(tmp, n_len):
    paths = []
    for i, g in enumerate(list(range(0, 5)) + [20, 21, 22, 40]):
        p = os.path.join(tmp, "c%d.fa" % i)
        orc.write_fasta(p, [orc.synth_genome(17, g, n_len)], names=["c%d" % i])
        paths.append(p)
    lst = os.path.join(tmp, "l.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst


def run_cli(binary, tmp, n_len, variants=()):
    lst = cluster_genomes(tmp, n_len)
    base = os.path.join(tmp, "plain.out")
    r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "-o", base], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ts = thresholds(base + ".matrix")
    got = {}
    for t in ts:
        out = os.path.join(tmp, "c.out")
        r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--matrix", "--cluster", "%.6f" % t, "-o", out], capture_output=True,
                           env=dict(os.environ, ANI_CLI_TRACE="1"))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"clusters written" in r.stderr
        assert open(out, "rb").read() == open(base, "rb").read()                       # -o and .matrix unchanged
        assert open(out + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
        got[t] = open(out + ".clusters").read()
        assert got[t] == clusters_from_matrix(base + ".matrix", np.float32("%.6f" % t)), t
    reps = [len({l.split("\t")[1] for l in c.splitlines()}) for c in got.values()]
    assert max(reps) > min(reps), reps                             # the thresholds do cut the genomes differently
    for bad in ("0", "150", "-3", "x"):
        r = subprocess.run([binary, "--ql", lst, "--rl", lst, "--cluster", bad, "-o", os.path.join(tmp, "bad.out")], capture_output=True)
        assert r.returncode == 1 and b"ERROR, --cluster" in r.stderr, bad
    # the same clusters through the other paths of the command line
    for name, args in variants:
        t = ts[len(ts) // 2]
        out = os.path.join(tmp, "v_%s.out" % name)
        r = subprocess.run([binary] + [a.replace("@L", lst).replace("@T", tmp) for a in args] + ["--cluster", "%.6f" % t, "-o", out],
                           capture_output=True)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert open(out + ".clusters").read() == got[t], name
    return got


# the same clusters through a saved reference sketch, --gpus 1, several reader threads, and -s
VARIANTS = [("save", ["--ql", "@L", "--rl", "@L", "--saveSketch", "@T/refs.anisk"]),
            ("sketch", ["--ql", "@L", "--refSketch", "@T/refs.anisk"]),
            ("gpus1", ["--ql", "@L", "--rl", "@L", "--gpus", "1"]),
            ("threads", ["--ql", "@L", "--rl", "@L", "-t", "3", "--matrix"]),
            ("sanity", ["--ql", "@L", "--rl", "@L", "-s"])]


def test_cli_cluster_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 30000, VARIANTS)


@pytest.mark.gpu
def test_cli_cluster_gpu(tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, str(tmp_path), 200000, VARIANTS)
