"""Single-linkage tree with the sketch fill, streamed (ani_tree_single_sketch, Engine.tree_single_sketch, fastANI --tree --treeMethod
single --treeFill sketch beyond 65 536 genomes) against the composition that defines it: ani_signature_pairs, the command line's fill
rule, ani_tree_single.  Every comparison is exact.
CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from fastani_amd.api import CGI_DT, AniError
from test_cluster import make_rows, pair_weights
from test_sigdist import identity_expected, make_signatures, pair_expected, two_genera
from test_tree_single import Linkage, kruskal, leaf_distances, missing_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
STRIP = "ANI_TEST_SIG_STRIP_ROWS"
STRIPS = (None, 1, 7, 16, 17, 64)          # unset, one row, a ragged strip, one tile, a tile and a row, more than n


def set_strip(monkeypatch, rows):
    if rows is None:
        monkeypatch.delenv(STRIP, raising=False)
    else:
        monkeypatch.setenv(STRIP, str(rows))


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition: signature_pairs -> the fill rule -> tree_single
# ---------------------------------------------------------------------------------------------------------------------------------
def composition(engine, rows, n, sig, length, k, min_shared, missing):
    """-> linkage, edges, source of ani_abi.h's rules 1 and 2"""
    pairs = engine.signature_pairs(sig, length, k, min_shared)
    q, r = rows["qryGenomeId"].astype(np.int64), rows["refGenomeId"].astype(np.int64)
    have = set(zip(np.minimum(q, r)[q != r].tolist(), np.maximum(q, r)[q != r].tolist()))
    fill = [(int(p["a"]), int(p["b"]), p["identity"]) for p in pairs if p["identity"] > 0 and (int(p["a"]), int(p["b"])) not in have]
    z, edges = engine.tree_single(np.concatenate([rows, make_rows(fill)]), n, missing, return_edges=True)
    filled = {(a, b) for a, b, _ in fill}
    at_missing = z[:, 2].astype(np.float32).view(np.uint32) == missing_distance(missing).view(np.uint32)
    source = np.array([2 if m else 1 if (a, b) in filled else 0 for (a, b), m in zip(edges.tolist(), at_missing.tolist())], dtype=np.uint8)
    return z, edges, source


def same(got, want):
    z, edges, source = got
    wz, wedges, wsource = want
    assert z.dtype == np.float64 and edges.dtype == np.int64 and source.dtype == np.uint8
    assert np.array_equal(z[:, :2], wz[:, :2]) and np.array_equal(z[:, 3], wz[:, 3])
    assert np.array_equal(z[:, 2].astype(np.float32).view(np.uint32), wz[:, 2].astype(np.float32).view(np.uint32))      # heights by bit pattern
    assert np.array_equal(z[:, 2].astype(np.float32).astype(np.float64), z[:, 2])
    assert np.array_equal(edges, wedges)
    assert np.array_equal(source, wsource)


def mixed_rows(rng, n, m):
    """duplicates, both directions, self rows, identities 60 ... 100"""
    q, r = rng.integers(0, n, m), rng.integers(0, n, m)
    q[:m // 5], r[:m // 5] = r[m // 2:m // 2 + m // 5], q[m // 2:m // 2 + m // 5]           # the other direction of some pairs
    q[m // 5:m // 5 + 6] = r[m // 5:m // 5 + 6]                                                # self rows
    rows = np.zeros(m, dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = q, r
    rows["identity"] = rng.uniform(60, 100, m).astype(np.float32)
    return rows[rng.permutation(m)]


def equals_composition(engine, monkeypatch):
    rng = np.random.default_rng(41)
    n, size = 40, 16
    sig, length = make_signatures([rng.choice(60, size=int(rng.integers(0, 26)), replace=False) * 70001 for _ in range(n)], size)
    rows = mixed_rows(rng, n, 150)
    lo, hi, _ = pair_weights(rows)
    assert len(lo) < len(rows) - 6 and (length == 0).any() and (length == size).any()
    seen = set()
    for min_shared in (1, 3):
        for missing in (0.0, 50.0):
            set_strip(monkeypatch, None)
            want = composition(engine, rows, n, sig, length, 16, min_shared, missing)
            seen |= set(want[2].tolist())
            for strip in STRIPS:
                set_strip(monkeypatch, strip)
                same(engine.tree_single_sketch(rows, n, sig, length, 16, min_shared, missing, return_edges=True, return_source=True), want)
                strips = engine.tree_single_sketch_strips()
                assert len(strips) == (1 if strip is None else -(-(n - 1) // min(strip, n - 1))), (strip, strips)
            # without the extras: the same linkage
            assert np.array_equal(engine.tree_single_sketch(rows, n, sig, length, 16, min_shared, missing), want[0])
    assert seen >= {0, 1}
    # rows only between a few genomes and little sharing: all three sources in one tree
    sig2, len2 = make_signatures([np.arange(g // 4 * 100, g // 4 * 100 + 16) + (g % 4) * 5 for g in range(n)], size)
    rows2 = make_rows([(0, 1, 97.0), (1, 0, 96.0), (5, 9, 91.5), (9, 13, 88.0), (4, 5, 62.0), (30, 30, 100.0)])
    for missing in (0.0, 50.0):
        set_strip(monkeypatch, None)
        want = composition(engine, rows2, n, sig2, len2, 16, 1, missing)
        assert set(want[2].tolist()) == {0, 1, 2}
        for strip in STRIPS:
            set_strip(monkeypatch, strip)
            same(engine.tree_single_sketch(rows2, n, sig2, len2, 16, 1, missing, return_edges=True, return_source=True), want)
    # size 1100: the 8 x 8 tiles
    n, size = 12, 1100
    sig, length = make_signatures([rng.choice(4000, size=int(rng.integers(900, 1500)), replace=False) * 1000003 for _ in range(n)], size)
    rows = mixed_rows(rng, n, 20)
    set_strip(monkeypatch, None)
    want = composition(engine, rows, n, sig, length, 16, 1, 0.0)
    assert 1 in want[2]
    for strip in (None, 1, 7, 8, 9):
        set_strip(monkeypatch, strip)
        same(engine.tree_single_sketch(rows, n, sig, length, 16, 1, 0.0, return_edges=True, return_source=True), want)


def test_equals_composition_cpu_build(emu_engine, monkeypatch):
    equals_composition(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_equals_composition_gpu(gpu_engine, monkeypatch):
    equals_composition(gpu_engine, monkeypatch)


def ties(engine, monkeypatch):
    """three groups of ten with one signature each and no rows: inside a group every pair is at distance 0, and the groups share three
    values of their eight two by two; equal distances merge in (lo, hi) order"""
    n, size = 30, 8
    base = [np.arange(0, 8), np.arange(5, 13), np.arange(10, 18)]
    sig, length = make_signatures([base[g % 3] * 1000 for g in range(n)], size)
    rows = make_rows([])
    set_strip(monkeypatch, None)
    want = composition(engine, rows, n, sig, length, 16, 1, 0.0)
    # the order, stated directly: Kruskal over every pair that shares something, ascending (bits(d), lo, hi)
    a, b = np.triu_indices(n, 1)
    shared = np.where(a % 3 == b % 3, 8, np.where((a % 3 + b % 3) == 2, 0, 3))                  # groups 0 and 2 share nothing
    keep = shared > 0
    w = np.array([identity_expected(int(s), 8, 16) for s in shared[keep]], dtype=np.float32)
    link = Linkage(n)
    kruskal(link, a[keep], b[keep], leaf_distances(w, 0.0))
    children, height, edges = link.result()
    assert np.array_equal(want[1], edges) and np.array_equal(want[0][:, :2].astype(np.int64), children)
    assert (height[:27] == 0).all() and height[27] > 0 and edges[:27].tolist() == [[g, g + 3 * i] for g in range(3) for i in range(1, 10)]
    assert (want[2] == 1).all()
    for strip in STRIPS:
        set_strip(monkeypatch, strip)
        same(engine.tree_single_sketch(rows, n, sig, length, 16, 1, 0.0, return_edges=True, return_source=True), want)


def test_ties_cpu_build(emu_engine, monkeypatch):
    ties(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_ties_gpu(gpu_engine, monkeypatch):
    ties(gpu_engine, monkeypatch)


def real_pair_masks(engine, monkeypatch):
    sig, length = make_signatures([np.arange(1, 9), np.arange(1, 9)], 8)
    rows = make_rows([(1, 0, 70.0)])
    for strip in (None, 1):
        set_strip(monkeypatch, strip)
        z, edges, source = engine.tree_single_sketch(rows, 2, sig, length, 16, 1, 0.0, return_edges=True, return_source=True)
        assert z.tolist() == [[0.0, 1.0, float(leaf_distances(np.float32([70.0]), 0.0)[0]), 2.0]] and edges.tolist() == [[0, 1]] and source.tolist() == [0]
        # the row's distance is not below the missing distance: the pair is a pair without rows, and still no sketch pair
        z, edges, source = engine.tree_single_sketch(rows, 2, sig, length, 16, 1, 80.0, return_edges=True, return_source=True)
        assert z.tolist() == [[0.0, 1.0, float(missing_distance(80.0)), 2.0]] and edges.tolist() == [[0, 1]] and source.tolist() == [2]
        # without the row the sketch pair is the merge, at distance 0
        z, edges, source = engine.tree_single_sketch(make_rows([(1, 1, 99.0)]), 2, sig, length, 16, 1, 80.0, return_edges=True, return_source=True)
        assert z.tolist() == [[0.0, 1.0, 0.0, 2.0]] and source.tolist() == [1]
        same((z, edges, source), composition(engine, make_rows([(1, 1, 99.0)]), 2, sig, length, 16, 1, 80.0))


def test_real_pair_masks_cpu_build(emu_engine, monkeypatch):
    real_pair_masks(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_real_pair_masks_gpu(gpu_engine, monkeypatch):
    real_pair_masks(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# above the ceiling of the pair step
# ---------------------------------------------------------------------------------------------------------------------------------
def grouped_input(n=66000, size=4):
    """genome g holds four values of a range private to its group g // 3: the group's members share 4, 2 or 1 values two by two, and
    genomes of different groups share nothing.  2000 rows chain some of the groups."""
    rng = np.random.default_rng(77)
    g = np.arange(n, dtype=np.int64)
    group, member = g // 3, g % 3
    # values 0..9 of the group's range: member 0 {0 1 2 3}, member 1 {0 1 4 5}: 2 shared with 0, member 2 {0 6 7 8}: 1 shared with both;
    # every fifth group has three identical members (4 shared)
    offsets = np.array([[0, 1, 2, 3], [0, 1, 4, 5], [0, 6, 7, 8]], dtype=np.int64)[member]
    offsets[(group % 5 == 0)] = [0, 1, 2, 3]
    sig = (group[:, None] * 16 + offsets + 1).astype(np.uint32)
    length = np.full(n, size, dtype=np.int32)
    a = rng.integers(0, n - 3, 2000)
    b = np.where(rng.random(2000) < 0.7, a + 3, a + 1)                                          # the next group, or the same one
    rows = np.zeros(2000, dtype=CGI_DT)
    flip = rng.random(2000) < 0.5
    rows["qryGenomeId"], rows["refGenomeId"] = np.where(flip, b, a), np.where(flip, a, b)
    rows["identity"] = rng.uniform(75, 100, 2000).astype(np.float32)
    return sig, length, rows


def grouped_expected(sig, length, rows, k):
    """test_tree_single's sparse restatement over the rows and the pairs inside the groups"""
    n = len(sig)
    lo, hi, w = pair_weights(rows)
    have = set(zip(lo.tolist(), hi.tolist()))
    assert n % 3 == 0
    flo, fhi, fw = [], [], []
    rel = (sig.astype(np.int64) - (np.arange(n) // 3 * 16)[:, None]).tolist()                  # a group's pairs repeat: one estimate per pattern
    memo = {}
    for first in range(0, n, 3):
        for a, b in ((first, first + 1), (first, first + 2), (first + 1, first + 2)):
            if (a, b) in have:
                continue
            key = (tuple(rel[a]), tuple(rel[b]))
            if key not in memo:
                sh, sz = pair_expected(sig[a], sig[b], 4)
                memo[key] = identity_expected(sh, sz, k) if sh else None
            if memo[key] is not None:
                flo.append(a), fhi.append(b), fw.append(memo[key])
    assert len(memo) >= 4
    all_lo = np.concatenate([lo, np.array(flo, dtype=np.int64)])
    all_hi = np.concatenate([hi, np.array(fhi, dtype=np.int64)])
    d = leaf_distances(np.concatenate([w, np.array(fw, dtype=np.float32)]), 0.0)
    from_sketch = np.concatenate([np.zeros(len(lo), dtype=bool), np.ones(len(flo), dtype=bool)])
    real = d.view(np.uint32) < missing_distance(0.0).view(np.uint32)
    link = Linkage(n)
    kruskal(link, all_lo[real], all_hi[real], d[real])
    forest = len(link.children)
    for leaf in range(1, n):
        link.merge(0, leaf, missing_distance(0.0))
    children, height, edges = link.result()
    sketchy = set(zip(all_lo[from_sketch].tolist(), all_hi[from_sketch].tolist()))
    source = np.array([1 if (a, b) in sketchy else 0 for a, b in edges[:forest].tolist()] + [2] * (n - 1 - forest), dtype=np.uint8)
    return children, height, edges, source


@pytest.mark.gpu
def test_above_the_old_ceiling_gpu(gpu_engine, monkeypatch):
    n = 66000
    sig, length, rows = grouped_input(n)
    children, height, edges, source = grouped_expected(sig, length, rows, 16)
    assert set(source.tolist()) == {0, 1, 2} and len(np.unique(height)) > 4
    for strip, strips in ((8192, 9), (None, None)):
        set_strip(monkeypatch, strip)
        z, got_edges, got_source = gpu_engine.tree_single_sketch(rows, n, sig, length, 16, 1, 0.0, return_edges=True, return_source=True)
        counts = gpu_engine.tree_single_sketch_strips()
        print("strip rows %s: %d strips, %d edges kept, %d rounds" % (strip, len(counts), int(counts.sum()), gpu_engine.tree_single_rounds()))
        assert strips is None or len(counts) == strips
        assert np.array_equal(z[:, :2].astype(np.int64), children)
        assert np.array_equal(z[:, 2].astype(np.float32).view(np.uint32), height.view(np.uint32))
        assert np.array_equal(got_edges, edges) and np.array_equal(got_source, source)
    # the pair step keeps its ceiling
    with pytest.raises(AniError) as ex:
        gpu_engine.signature_pairs(sig, length, 16, 1)
    assert ex.value.code == -4


# ---------------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    rows = make_rows([(0, 1, 97.0), (1, 2, 96.0)])
    lib, h = engine.lib, engine.h
    ch, ht, ed, src = np.full(4, -7, np.int32), np.full(2, -7, np.float32), np.full(4, -7, np.int32), np.full(2, 7, np.uint8)

    def call(n=3, size=3, k=16, ms=1, missing=0.0, rows_p=rows.ctypes.data, n_rows=2, sig_p=sig.ctypes.data, len_p=length.ctypes.data, ch_p=ch.ctypes.data,
             ht_p=ht.ctypes.data, ed_p=ed.ctypes.data, src_p=src.ctypes.data, ctx=h):
        return lib.ani_tree_single_sketch(ctx, rows_p, n_rows, n, ctypes.c_float(missing), sig_p, len_p, size, k, ms, ch_p, ht_p, ed_p, src_p)

    assert call() == 0 and call(ed_p=None) == 0 and call(src_p=None) == 0 and call(ed_p=None, src_p=None) == 0
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for k in (0, -3, 17):
        assert call(k=k) == -1, k
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for missing in (-1.0, 100.5, float("nan")):
        assert call(missing=missing) == -1, missing
    assert call(n=-1) == -1
    assert call(sig_p=None) == -1 and call(len_p=None) == -1 and call(ch_p=None) == -1 and call(ht_p=None) == -1 and call(rows_p=None) == -1
    assert call(ctx=None) == -1
    assert call(n=(1 << 30) + 1) == -4                                 # the limits, before anything is read or allocated
    assert call(n_rows=1 << 32) == -4
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.tree_single_sketch(rows, 3, sig, np.array(bad_len, dtype=np.int32), 16)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.tree_single_sketch(rows, 3, x, length, 16)
        assert ex.value.code == -1, bad_row
    x = sig.copy()
    x[2] = [9, 9, 1]                                                   # beyond the length: not looked at
    assert np.array_equal(engine.tree_single_sketch(rows, 3, x, length, 16), engine.tree_single_sketch(rows, 3, sig, length, 16))
    for bad in ((0, 3, 97.0), (-1, 1, 97.0), (0, 2, 0.0), (0, 2, -3.0), (0, 2, 100.5), (1, 1, float("nan"))):
        for missing in (0.0, 100.0):                                  # the rows are checked whatever the missing identity leaves of them
            with pytest.raises(AniError) as ex:
                engine.tree_single_sketch(make_rows([(0, 1, 97.0), bad]), 3, sig, length, 16, 1, missing)
            assert ex.value.code == -1, bad
    # nGenomes of 0 and 1: ANI_OK, nothing read or written
    before = (ch.copy(), ht.copy(), ed.copy(), src.copy())
    for n in (0, 1):
        assert call(n=n) == 0 and call(n=n, n_rows=0, rows_p=None, sig_p=None, len_p=None, ch_p=None, ht_p=None, ed_p=None, src_p=None) == 0
        for got, want in zip((ch, ht, ed, src), before):
            assert np.array_equal(got, want)
        z, edges, source = engine.tree_single_sketch(make_rows([]), n, np.zeros((n, 5), np.uint32), np.zeros(n, np.int32), 16, return_edges=True, return_source=True)
        assert z.shape == (0, 4) and edges.shape == (0, 2) and source.shape == (0,)
    # missing identity 100: every merge is a join to leaf 0 at height 0
    z, edges, source = engine.tree_single_sketch(rows, 3, sig, length, 16, 1, 100.0, return_edges=True, return_source=True)
    assert z[:, 2].tolist() == [0.0, 0.0] and edges.tolist() == [[0, 1], [0, 2]] and source.tolist() == [2, 2]


def test_errors_cpu_build(emu_engine):
    argument_errors(emu_engine)


@pytest.mark.gpu
def test_errors_gpu(gpu_engine):
    argument_errors(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
STREAM = {"ANI_TEST_CLI_SINGLE_STREAM": "1", STRIP: "2"}
EXTS = ("", ".matrix", ".newick", ".mst")


def run(binary, args, env=None):
    return subprocess.run([binary] + args, capture_output=True, env=dict(os.environ, **(env or {})))


def read_all(base, exts=EXTS):
    return {ext: open(base + ext, "rb").read() for ext in exts}


def run_cli(binary, tmp, n_len):
    lst, paths, _ = two_genera(tmp, n_len)
    tree = ["--tree", "--treeMethod", "single", "--treeFill", "sketch", "--sketchSize", "2000", "--matrix"]
    plain, streamed = os.path.join(tmp, "plain.out"), os.path.join(tmp, "streamed.out")
    r = run(binary, ["--ql", lst, "--rl", lst] + tree + ["-o", plain], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"sketch pairs compared" in r.stderr and b"sketch pairs folded" not in r.stderr
    r = run(binary, ["--ql", lst, "--rl", lst] + tree + ["-o", streamed], dict(STREAM, ANI_CLI_TRACE="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"sketch pairs folded" in r.stderr and b"sketch pairs compared" not in r.stderr
    want = read_all(plain)
    assert read_all(streamed) == want
    sources = [ln.split("\t")[3] for ln in want[".mst"].decode().splitlines()]
    assert "sketch" in sources and "ani" in sources
    # a reference sketch file in blocks of genomes, and two device contexts
    skf = os.path.join(tmp, "refs.anisk")
    assert run(binary, ["--ql", lst, "--rl", lst, "--saveSketch", skf, "-o", os.path.join(tmp, "save.out")]).returncode == 0
    blocks = os.path.join(tmp, "blocks.out")
    r = run(binary, ["--ql", lst, "--refSketch", skf] + tree + ["-o", blocks], dict(STREAM, ANI_CLI_REF_BLOCK_BYTES="30000"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"blocks of genomes per device" in r.stderr
    assert read_all(blocks) == want
    devices = os.path.join(tmp, "devices.out")
    r = run(binary, ["--ql", lst, "--rl", lst, "--devices", "0,0"] + tree + ["-o", devices], STREAM)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert read_all(devices) == want
    # --sketchANI keeps the pair step, variable or not: the same files, .sketch among them
    exts = EXTS + (".sketch",)
    s0, s1 = os.path.join(tmp, "s0.out"), os.path.join(tmp, "s1.out")
    for o, env in ((s0, {"ANI_CLI_TRACE": "1"}), (s1, dict(STREAM, ANI_CLI_TRACE="1"))):
        r = run(binary, ["--ql", lst, "--rl", lst, "--sketchANI"] + tree + ["-o", o], env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"sketch pairs compared" in r.stderr and b"sketch pairs folded" not in r.stderr
    assert read_all(s1, exts) == read_all(s0, exts) and read_all(s0) == want
    # the other tree methods are not streamed either
    for method in ("average", "nj"):
        a, b = os.path.join(tmp, method + "0.out"), os.path.join(tmp, method + "1.out")
        args = ["--ql", lst, "--rl", lst, "--tree", "--treeMethod", method, "--treeFill", "sketch", "--sketchSize", "2000"]
        assert run(binary, args + ["-o", a]).returncode == 0 and run(binary, args + ["-o", b], STREAM).returncode == 0
        assert read_all(a, ("", ".newick")) == read_all(b, ("", ".newick")) and not os.path.exists(b + ".mst")


def ceiling_refusals(binary, tmp):
    """65 537 references: --sketchANI and the dense methods are refused before anything is read, as before; the single-linkage tree
    passes that check"""
    p = os.path.join(tmp, "g.fa")
    open(p, "w").write(">c\nACGT\n")
    names = [os.path.join(tmp, "x%d.fa" % i) for i in range(65537)]
    for x in names:
        os.symlink(p, x)
    many, one, other = os.path.join(tmp, "many.txt"), os.path.join(tmp, "one.txt"), os.path.join(tmp, "other.txt")
    open(many, "w").write("\n".join(names) + "\n")
    open(one, "w").write(names[0] + "\n")
    open(other, "w").write(p + "\n")
    bad = os.path.join(tmp, "bad.out")
    msg = b"ERROR, --sketchANI and --treeFill sketch take at most 65536 genomes, this run has 65537"
    single = ["--tree", "--treeMethod", "single", "--treeFill", "sketch"]
    for extra in (["--sketchANI"], ["--tree", "--treeFill", "sketch"], ["--tree", "--treeMethod", "nj", "--treeFill", "sketch"], single + ["--sketchANI"]):
        for env in ({}, STREAM):
            r = run(binary, ["--ql", one, "--rl", many] + extra + ["-o", bad], dict(env, ANI_CLI_TRACE="1"))
            assert r.returncode == 1 and msg in r.stderr and b"devices initialised" not in r.stderr, (extra, r.stderr[-300:])
    # the single-linkage tree alone goes on to the next check of the same function (a query outside the references ends the run there)
    r = run(binary, ["--ql", other, "--rl", many] + single + ["-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and msg not in r.stderr and b"is not among the references" in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    assert not os.path.exists(bad)


def test_cli_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 50000)


def test_cli_ceiling_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    ceiling_refusals(os.path.join(EMU, "fastANI_emu"), str(tmp_path))


@pytest.mark.gpu
def test_cli_gpu(tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    for sub in ("a", "b"):
        os.mkdir(os.path.join(str(tmp_path), sub))
    run_cli(binary, os.path.join(str(tmp_path), "a"), 200000)
    ceiling_refusals(binary, os.path.join(str(tmp_path), "b"))
