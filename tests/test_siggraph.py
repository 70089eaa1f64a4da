"""The streamed sketch pair graph (ani_signature_graph, Engine.signature_graph, fastANI --sketchGraph) against what defines it
(include/ani_abi.h, rules 1 - 7).  Mash estimate: the pairs of ani_signature_pairs, or pair_expected / identity_expected of
test_sigdist, kept by the bit pattern of their identity.  Containment estimate: cell_expected, denominator and identity_expected of
test_sigcontain in mode MAX over every a < b.  Every comparison is exact: a, b, shared, size, identity bits, order and count.  The
expected records never come from the call under test.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu):
the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_sigcontain as contain
from fastani_amd.api import SIGPAIR_DT, AniError
from test_cluster import read_matrix
from test_sigdist import identity_expected, make_signatures, pair_expected, random_sets, two_genera
from test_signeighbors import EMU, ROOT, STRIP, STRIPS, bits, run, set_strip, strips_of

MASH, CONTAIN = 0, 1
GRAPH_ROWS = "ANI_TEST_CLI_GRAPH_ROWS"


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition: rules 1 - 4
# ---------------------------------------------------------------------------------------------------------------------------------
def low_bits(min_identity):
    return bits(0.0 if min_identity == 0 else min_identity)


def kept(pairs, min_identity, begin, end):
    """rules 3 and 4 over a SIGPAIR_DT array in (a, b) order"""
    return pairs[(pairs["identity"].view(np.uint32) >= low_bits(min_identity)) & (pairs["a"] >= begin) & (pairs["a"] < end)]


def cells_expected(sig, length, estimate, rows):
    """(a, b, shared, size-or-d) of every pair a < b with a in `rows`, restated: rule 2 of ani_signature_pairs, or rules 1 - 4 of
    ani_signature_screen_contain in mode MAX with a's signature as Q and b's as R"""
    n, size = sig.shape
    out = []
    for a in rows:
        x = sig[a, :length[a]]
        for b in range(a + 1, n):
            y = sig[b, :length[b]]
            if estimate == MASH:
                out.append((a, b) + pair_expected(x, y, size))
            else:
                cell = contain.cell_expected(x, y, size)
                out.append((a, b, cell[0], contain.denominator(cell, contain.MAX)))
    return out


def records_expected(cells, estimate, kmer, min_shared, min_identity):
    """rules 1 - 3 over the cells -> SIGPAIR_DT array"""
    ident = identity_expected if estimate == MASH else contain.identity_expected
    out = [(a, b, sh, sz, ident(sh, sz, kmer)) for a, b, sh, sz in cells if sh >= min_shared]
    return kept(np.array(out, dtype=SIGPAIR_DT), min_identity, 0, 1 << 31)


def same(got, want):
    assert got.dtype == SIGPAIR_DT and got.shape == want.shape, (got.shape, want.shape)
    for f in ("a", "b", "shared", "size"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["identity"].view(np.uint32), want["identity"].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. composition
# ---------------------------------------------------------------------------------------------------------------------------------
def composition_input():
    rng = np.random.default_rng(41)
    n, size = 40, 16
    sig, length = make_signatures([rng.choice(60, size=int(rng.integers(0, 26)), replace=False) * 70001 for _ in range(n)], size)
    assert (length == 0).any() and (length == size).any()
    return n, sig, length


def composition(engine, monkeypatch):
    """Of the three kinds of rows the cases are to contain, this input has two: a row without a kept pair and a row that the threshold
    cuts.  It has no row with all pairs kept and at least one pair: genome 37 is empty and genomes 38 and 39 share nothing, so every row
    before them lacks a pair.  That kind is asserted in dense_ties, whose middle group shares values with every genome."""
    n, sig, length = composition_input()
    shareds, idents, kmers, ranges = (1, 3), (0.0, 70.0, 100.0, -0.0), (16, 9), ((0, 40), (5, 23), (39, 40), (7, 7))
    set_strip(monkeypatch, None)
    pairs = {(k, ms): engine.signature_pairs(sig, length, k, ms) for k in kmers for ms in shareds}
    cells = cells_expected(sig, length, CONTAIN, range(n))
    seen = {"empty": False, "cut": False}

    def want(est, k, ms, mi, begin, end):
        if est == MASH:
            w = kept(pairs[(k, ms)], mi, begin, end)
        else:
            w = kept(records_expected(cells, CONTAIN, k, ms, mi), mi, begin, end)
        per_row = np.bincount(w["a"], minlength=n)
        for a in range(begin, min(end, n - 1)):
            seen["empty"] |= per_row[a] == 0
            seen["cut"] |= 0 < per_row[a] < n - 1 - a and mi != 0
        return w

    # every estimate, k-mer size, minShared and minIdentity at the default strip height, all rows
    for est in (MASH, CONTAIN):
        for k in kmers:
            for ms in shareds:
                for mi in idents:
                    same(engine.signature_graph(sig, length, k, mi, ms, est), want(est, k, ms, mi, 0, n))
                    assert engine.signature_graph_strips() == 1
    # every strip height with every row range; the other parameters take turns
    turn = 0
    for strip in STRIPS:
        for begin, end in ranges:
            ms, mi, k, est = shareds[turn % 2], idents[(turn // 2) % 4], kmers[(turn // 3) % 2], (MASH, CONTAIN)[(turn // 5) % 2]
            turn += 1
            set_strip(monkeypatch, strip)
            same(engine.signature_graph(sig, length, k, mi, ms, est, rows=(begin, end)), want(est, k, ms, mi, begin, end))
            assert engine.signature_graph_strips() == strips_of(strip, end - begin), (strip, begin, end)
    assert seen["empty"] and seen["cut"], seen
    # at the Mash estimate, threshold 0 and all rows: the records of signature_pairs
    for strip in (None, 7):
        set_strip(monkeypatch, strip)
        for k, ms in pairs:
            got = engine.signature_graph(sig, length, k, 0.0, ms, "mash")
            assert np.array_equal(got, pairs[(k, ms)]) and len(got) > 100
    # the names of the estimates
    same(engine.signature_graph(sig, length, 16, 70.0, estimate="contain"), engine.signature_graph(sig, length, 16, 70.0, estimate=1))
    with pytest.raises(ValueError):
        engine.signature_graph(sig, length, 16, 70.0, estimate="jaccard")


def test_composition_cpu_build(emu_engine, monkeypatch):
    composition(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_composition_gpu(gpu_engine, monkeypatch):
    composition(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. split ranges
# ---------------------------------------------------------------------------------------------------------------------------------
def split_ranges(engine, monkeypatch):
    n, sig, length = composition_input()
    set_strip(monkeypatch, 7)
    for est in (MASH, CONTAIN):
        whole = engine.signature_graph(sig, length, 16, 70.0, 1, est)
        parts = [engine.signature_graph(sig, length, 16, 70.0, 1, est, rows=r) for r in ((0, 13), (13, 14), (14, 40))]
        assert all(len(p) for p in parts)
        same(np.concatenate(parts), whole)
        same(whole, records_expected(cells_expected(sig, length, est, range(n)), est, 16, 1, 70.0))


def test_split_ranges_cpu_build(emu_engine, monkeypatch):
    split_ranges(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_split_ranges_gpu(gpu_engine, monkeypatch):
    split_ranges(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. pitch classes and tile edges
# ---------------------------------------------------------------------------------------------------------------------------------
PITCH_CASES = ((16, 37, 16), (1000, 21, 16), (2048, 13, 8), (4096, 9, 4))          # size, genomes, tile edge


def pitch_classes(engine, monkeypatch, size, n, edge):
    assert n % edge != 0
    rng = np.random.default_rng(45 + size)
    sig, length = make_signatures(random_sets(rng, n, size, 8 * size), size)
    begin, end = 1, n - 2                                              # off a tile edge at either end
    assert begin % edge and end % edge and end - begin > edge
    for est in (MASH, CONTAIN):
        cells = cells_expected(sig, length, est, range(begin, end))
        everything = records_expected(cells, est, 16, 1, 0.0)
        for mi in (0.0, float(np.sort(everything["identity"])[len(everything) // 2])):     # no threshold, and the median of the expected estimates
            want = records_expected(cells, est, 16, 1, mi)
            assert 0 < len(want) and (mi == 0 or len(want) < len(everything))
            for strip in (5, None):
                set_strip(monkeypatch, strip)
                same(engine.signature_graph(sig, length, 16, mi, 1, est, rows=(begin, end)), want)
                assert engine.signature_graph_strips() == strips_of(strip, end - begin)


@pytest.mark.parametrize("size,n,edge", PITCH_CASES)
def test_pitch_classes_cpu_build(emu_engine, monkeypatch, size, n, edge):
    pitch_classes(emu_engine, monkeypatch, size, n, edge)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n,edge", PITCH_CASES)
def test_pitch_classes_gpu(gpu_engine, monkeypatch, size, n, edge):
    pitch_classes(gpu_engine, monkeypatch, size, n, edge)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dense and ties
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_ties(engine, monkeypatch):
    """three groups of ten with one signature each: twins at 100, the groups next to each other at 3 shared of 8, groups 0 and 2 share
    nothing"""
    n, size = 30, 8
    base = [np.arange(0, 8), np.arange(5, 13), np.arange(10, 18)]
    sig, length = make_signatures([base[g % 3] * 1000 for g in range(n)], size)
    twins = [(a, b, 8, 8, np.float32(100.0)) for a in range(n) for b in range(a + 1, n) if a % 3 == b % 3]
    near = identity_expected(3, 8, 16)
    every = [(a, b, 8, 8, np.float32(100.0)) if a % 3 == b % 3 else (a, b, 3, 8, near) for a in range(n) for b in range(a + 1, n) if abs(a % 3 - b % 3) != 2]
    assert len(twins) == 3 * 45 and 0 < bits(near) < bits(100.0)
    cells = cells_expected(sig, length, CONTAIN, range(n))
    for strip in (1, None):
        set_strip(monkeypatch, strip)
        same(engine.signature_graph(sig, length, 16, 100.0), np.array(twins, dtype=SIGPAIR_DT))
        got = engine.signature_graph(sig, length, 16, 0.0)
        same(got, np.array(every, dtype=SIGPAIR_DT))
        per_row = np.bincount(got["a"], minlength=n)
        assert per_row[1] == 28 and per_row[4] == 25 and per_row[0] == 19                          # rows with all pairs kept, and one without
        for mi in (100.0, 0.0):
            same(engine.signature_graph(sig, length, 16, mi, estimate="contain"), records_expected(cells, CONTAIN, 16, 1, mi))


def test_dense_ties_cpu_build(emu_engine, monkeypatch):
    dense_ties(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_dense_ties_gpu(gpu_engine, monkeypatch):
    dense_ties(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. containment differs where it should
# ---------------------------------------------------------------------------------------------------------------------------------
def containment_differs(engine, monkeypatch):
    """a complete small genome inside a large one: all of its four values are in the large one's sketch"""
    full = np.arange(1, 17) * 1001
    sig, length = make_signatures([full, full[[2, 5, 9, 14]]], 16)
    assert length.tolist() == [16, 4]
    set_strip(monkeypatch, None)
    for order in ((0, 1), (1, 0)):                                     # symmetric: which genome is Q does not matter
        s, l = sig[list(order)], length[list(order)]
        got = engine.signature_graph(s, l, 16, 0.0, estimate="contain")
        assert got.tolist() == [(0, 1, 4, 4, 100.0)]
        got = engine.signature_graph(s, l, 16, 0.0, estimate="mash")
        w = identity_expected(4, 16, 16)
        assert got[["a", "b", "shared", "size"]].tolist() == [(0, 1, 4, 16)] and bits(got["identity"][0]) == bits(w) and 0 < float(w) < 100
        assert len(engine.signature_graph(s, l, 16, 100.0, estimate="contain")) == 1 and len(engine.signature_graph(s, l, 16, 100.0, estimate="mash")) == 0


def test_containment_differs_cpu_build(emu_engine, monkeypatch):
    containment_differs(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_containment_differs_gpu(gpu_engine, monkeypatch):
    containment_differs(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. above the ceiling of the pair step
# ---------------------------------------------------------------------------------------------------------------------------------
def above_the_old_ceiling(engine, monkeypatch):
    n, size = 65537, 2
    kinds = [(), (3,), (3, 9), (5, 9), (9, 11), (3, 5), (11,)]         # a handful of values: every genome is one of these sets
    kind = np.random.default_rng(46).integers(0, len(kinds), n)
    sig, length = np.zeros((n, size), np.uint32), np.zeros(n, np.int32)
    for i, s in enumerate(kinds):
        sig[kind == i, :len(s)] = s
        length[kind == i] = len(s)
    memo = {}

    def rows_expected(begin, end, min_identity):
        out = []
        for a in range(begin, end):
            for b in range(a + 1, n):
                key = (kind[a], kind[b])
                if key not in memo:
                    sh, sz = pair_expected(np.array(kinds[key[0]], np.uint32), np.array(kinds[key[1]], np.uint32), size)
                    memo[key] = (sh, sz, identity_expected(sh, sz, 16))
                if memo[key][0] >= 1:
                    out.append((a, b) + memo[key])
        return kept(np.array(out, dtype=SIGPAIR_DT), min_identity, begin, end)

    set_strip(monkeypatch, None)
    for (begin, end), mi in (((0, 2), 0.0), ((65530, 65537), 95.0)):
        want = rows_expected(begin, end, mi)
        assert len(want) > 0
        same(engine.signature_graph(sig, length, 16, mi, rows=(begin, end)), want)
        assert engine.signature_graph_strips() == 1
    # the pair step keeps its ceiling
    with pytest.raises(AniError) as ex:
        engine.signature_pairs(sig, length, 16, 1)
    assert ex.value.code == -4


def test_above_the_old_ceiling_cpu_build(emu_engine, monkeypatch):
    above_the_old_ceiling(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_above_the_old_ceiling_gpu(gpu_engine, monkeypatch):
    above_the_old_ceiling(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def arguments(engine):
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    lib, h = engine.lib, engine.h
    rows, m = ctypes.c_void_p(), ctypes.c_size_t()

    def call(n=3, size=3, kmer=16, ms=1, mi=0.0, est=0, begin=0, end=3, sig_p=sig.ctypes.data, len_p=length.ctypes.data, rows_p=ctypes.byref(rows),
             m_p=ctypes.byref(m), ctx=h):
        rows.value, m.value = 7, 7
        rc = lib.ani_signature_graph(ctx, sig_p, len_p, n, size, kmer, ms, ctypes.c_float(mi), est, begin, end, rows_p, m_p)
        if rc == 0 and rows_p is not None and rows.value:
            lib.ani_free(rows)
        return rc

    assert call() == 0 and m.value == 1
    assert call(est=1) == 0 and m.value == 1
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for kmer in (0, -3, 17):
        assert call(kmer=kmer) == -1, kmer
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for mi in (-1.0, 100.5, float("nan")):
        assert call(mi=mi) == -1, mi
    for est in (-1, 2):
        assert call(est=est) == -1, est
    for begin, end in ((-1, 2), (2, 1), (0, 4), (4, 4)):
        assert call(begin=begin, end=end) == -1, (begin, end)
    assert call(n=-1, begin=0, end=0) == -1
    assert call(sig_p=None) == -1 and call(len_p=None) == -1 and call(rows_p=None) == -1 and call(m_p=None) == -1 and call(ctx=None) == -1
    assert call(n=(1 << 30) + 1) == -4                                 # the limit, before anything is read or allocated
    assert call(n=(1 << 30) + 1, sig_p=None, len_p=None) == -4
    # the scalar checks fire with a null sig
    assert call(size=0, sig_p=None) == -1 and call(kmer=17, sig_p=None) == -1 and call(ms=0, sig_p=None) == -1 and call(mi=float("nan"), sig_p=None) == -1
    assert call(est=2, sig_p=None) == -1 and call(begin=2, end=1, sig_p=None) == -1
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.signature_graph(sig, np.array(bad_len, dtype=np.int32), 16)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.signature_graph(x, length, 16, rows=(2, 3))         # whatever the range: every signature is checked
        assert ex.value.code == -1, bad_row
    x = sig.copy()
    x[2] = [9, 9, 1]                                                   # beyond the length: not looked at
    same(engine.signature_graph(x, length, 16), engine.signature_pairs(sig, length, 16, 1))
    # an empty range, one genome or none: ANI_OK after the scalar checks, no rows, null arrays allowed
    for n, begin, end in ((3, 0, 0), (3, 2, 2), (3, 3, 3), (0, 0, 0), (1, 0, 1), (1, 0, 0)):
        assert call(n=n, begin=begin, end=end) == 0 and rows.value is None and m.value == 0
        assert call(n=n, begin=begin, end=end, sig_p=None, len_p=None) == 0 and rows.value is None and m.value == 0
        assert lib.ani_signature_graph_strips(h) == 0
        assert call(n=n, begin=begin, end=end, ms=0) == -1 and call(n=n, begin=begin, end=end, mi=float("nan")) == -1
    assert lib.ani_signature_graph_strips(None) == 0
    assert engine.signature_graph(np.zeros((0, 5), np.uint32), np.zeros(0, np.int32), 16).shape == (0,)
    got = engine.signature_graph(sig, length, 16, min_shared=3)        # a range without a kept pair
    assert got.shape == (0,) and got.dtype == SIGPAIR_DT and engine.signature_graph_strips() == 1


def test_arguments_cpu_build(emu_engine):
    arguments(emu_engine)


@pytest.mark.gpu
def test_arguments_gpu(gpu_engine):
    arguments(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def outputs(prefix):
    """{extension: bytes} of every file a run wrote"""
    d, base = os.path.split(prefix)
    return {f[len(base):]: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith(base)}


def run_cli(binary, engine, tmp, n_len):
    lst, paths, genomes = two_genera(tmp, n_len)
    common = ["--ql", lst, "--rl", lst, "--matrix"]
    size = 2000
    base = os.path.join(tmp, "base.out")
    assert run(binary, common + ["-o", base]).returncode == 0
    texts = {}
    for t in ("70", "95"):
        g, sk = os.path.join(tmp, "g%s.out" % t), os.path.join(tmp, "sk%s.out" % t)
        r = run(binary, common + ["--sketchGraph", t, "--sketchSize", str(size), "-o", g], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"sketch graph found" in r.stderr and b"sketch graph written" in r.stderr and b"sketch pairs compared" not in r.stderr
        assert run(binary, common + ["--sketchANI", "--sketchSize", str(size), "--sketchMinANI", t, "-o", sk]).returncode == 0
        texts[t] = open(g + ".sketchgraph", "rb").read()
        assert texts[t] == open(sk + ".sketch", "rb").read()
        # with the option every other file is what it was without it
        got, before = outputs(g), outputs(base)
        assert set(got) == set(before) | {".sketchgraph"} and ".sketch" not in got
        for ext in before:
            assert got[ext] == before[ext], ext
    names, _ = read_matrix(os.path.join(tmp, "g70.out.matrix"))
    assert names == paths
    assert 0 < len(texts["95"].splitlines()) < len(texts["70"].splitlines()) <= 15
    # the range height of the file and the strip height of the call change nothing
    for name, env in (("rows1", {GRAPH_ROWS: "1"}), ("rows3", {GRAPH_ROWS: "3"}), ("strip2", {STRIP: "2"})):
        o = os.path.join(tmp, name + ".out")
        r = run(binary, common + ["--sketchGraph", "70", "--sketchSize", str(size), "-o", o], env)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert open(o + ".sketchgraph", "rb").read() == texts["70"], name
    # the containment estimate: the lines of Engine.signature_graph on the signatures of the same genomes
    sig, length = contain.signatures_of(engine, genomes, size)
    o = os.path.join(tmp, "contain.out")
    r = run(binary, common + ["--sketchGraph", "70", "--sketchContain", "max", "--sketchSize", str(size), "-o", o])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    recs = engine.signature_graph(sig, length, 16, 70.0, 1, "contain")
    want = "".join("%s\t%s\t%s\t%d/%d\n" % (paths[x["a"]], paths[x["b"]], "%g" % x["identity"], x["shared"], x["size"]) for x in recs)
    assert open(o + ".sketchgraph").read() == want and len(recs) > 0
    # refusals, all before a device is touched
    bad = os.path.join(tmp, "bad.out")
    for t in ("0", "100.5", "-3", "x"):
        r = run(binary, common + ["--sketchGraph", t, "-o", bad], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 1 and b"ERROR, --sketchGraph takes an ANI threshold in (0, 100]" in r.stderr and b"devices initialised" not in r.stderr, (t, r.stderr[-300:])
    for mode in ("query", "reference"):
        r = run(binary, common + ["--sketchGraph", "90", "--sketchContain", mode, "-o", bad], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 1 and b"ERROR, --sketchGraph takes --sketchContain max only" in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    r = run(binary, common + ["--sketchContain", "max", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"ERROR, --sketchContain needs --sketchScreen" in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    few = os.path.join(tmp, "few.txt")
    open(few, "w").write("\n".join(paths[:4]) + "\n")
    r = run(binary, ["--ql", lst, "--rl", few, "--sketchGraph", "90", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"is not among the references" in r.stderr and paths[4].encode() in r.stderr, r.stderr[-500:]
    assert b"devices initialised" not in r.stderr
    assert not os.path.exists(bad) and not os.path.exists(bad + ".sketchgraph")
    assert b"--sketchGraph" in run(binary, ["-h"]).stdout


def ceiling(binary, tmp):
    """65 537 references: the option alone passes the ceiling check and goes on to the next check of the same function, where a query
    outside the references ends the run; with --sketchANI beside it the pair step's refusal stays"""
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
    r = run(binary, ["--ql", other, "--rl", many, "--sketchGraph", "90", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and msg not in r.stderr and b"is not among the references" in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    r = run(binary, ["--ql", one, "--rl", many, "--sketchGraph", "90", "--sketchANI", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and msg in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    assert not os.path.exists(bad)


def test_cli_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 50000)


def test_cli_ceiling_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    ceiling(os.path.join(EMU, "fastANI_emu"), str(tmp_path))


@pytest.mark.gpu
def test_cli_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    for sub in ("a", "b"):
        os.mkdir(os.path.join(str(tmp_path), sub))
    run_cli(binary, gpu_engine, os.path.join(str(tmp_path), "a"), 200000)
    ceiling(binary, os.path.join(str(tmp_path), "b"))
