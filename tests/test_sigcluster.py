"""Greedy representative clustering under the whole-genome sketch estimate (ani_signature_cluster, Engine.signature_cluster, fastANI
--sketchCluster T) against a plain-Python restatement of its rules 1 - 4 (include/ani_abi.h) over the numpy pair_expected /
identity_expected, written here, and against the composition that rule 5 names: engine.cluster_greedy over the rows of
engine.signature_pairs.  Every comparison is exact: ids, shared, size, identity by bit pattern, and the unused record of a
representative.  The expected values never come from the call under test.  CPU: the tests/emu build of the library and of the command
line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import fastani_amd
from fastani_amd.api import CGI_DT, NEIGHBOR_DT, AniError
from test_sigdist import identity_expected, make_signatures, pair_expected, random_sets, two_genera
from test_sigscreen import SHAPE, STRIP, bits, run, set_env, small_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
UNUSED = np.array((-1, 0, 0, 0.0), dtype=NEIGHBOR_DT)
identity_of = functools.lru_cache(maxsize=None)(identity_expected)


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def cells_of(sig, length):
    """rule 1: (shared, size) of every pair a < b, by numpy"""
    n, size = sig.shape
    return {(a, b): pair_expected(sig[a, :length[a]], sig[b, :length[b]], size) for a in range(n) for b in range(a + 1, n)}


@functools.lru_cache(maxsize=None)
def small_cells():
    sig, length = small_data()
    return sig, length, cells_of(sig, length)


def greedy_expected(cells, n, kmer, min_shared, min_identity):
    """rules 2 - 4 -> (representative, link, facts); facts counts what tells the rules apart: members whose representative has a larger
    id, members with two representatives tied at the best identity, representatives with an edge to an earlier member"""
    low = bits(min_identity)
    adj = [{} for _ in range(n)]
    for (a, b), (sh, sz) in cells.items():
        w = identity_of(sh, sz, kmer)
        if sh >= min_shared and bits(w) >= low:                       # rule 2
            adj[a][b] = adj[b][a] = (sh, sz, w)
    reps = []
    for i in range(n):                                                # rule 3: id order
        if not any(j in adj[i] for j in reps):
            reps.append(i)
    is_rep = set(reps)
    representative = np.arange(n, dtype=np.int32)
    link = np.zeros(n, dtype=NEIGHBOR_DT)
    link[:] = UNUSED
    facts = {"later": 0, "tied": 0, "chains": 0, "members": 0}
    for i in range(n):
        if i in is_rep:
            facts["chains"] += any(j < i and j not in is_rep for j in adj[i])
            continue
        near = sorted((-bits(adj[i][r][2]), r) for r in adj[i] if r in is_rep)
        assert near
        r = near[0][1]
        representative[i] = r
        link[i] = (r,) + adj[i][r]
        facts["members"] += 1
        facts["later"] += r > i
        facts["tied"] += len(near) > 1 and near[1][0] == near[0][0]
    return representative, link, facts


def same(got, want):
    (rep, link), (wrep, wlink) = got, want[:2]
    assert rep.dtype == np.int32 and link.dtype == NEIGHBOR_DT and rep.shape == wrep.shape and link.shape == wlink.shape
    assert np.array_equal(rep, wrep), (rep, wrep)
    for f in ("neighbor", "shared", "size"):
        assert np.array_equal(link[f], wlink[f]), f
    assert np.array_equal(link["identity"].view(np.uint32), wlink["identity"].view(np.uint32))
    own = rep == np.arange(len(rep))
    assert (link[own] == UNUSED).all() and (link["neighbor"][~own] == rep[~own]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the definition on the small set
# ---------------------------------------------------------------------------------------------------------------------------------
def definition_small(engine, monkeypatch):
    sig, length, cells = small_cells()
    n = len(sig)
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    first = min(r for r in range(n) if length[r] == length[11] and (sig[r] == sig[11]).all())
    told = set()
    for kmer in (16, 9):
        for ms in (1, 3):
            for t in (70.0, 85.0, 90.0, 95.0, 100.0):
                want = greedy_expected(cells, n, kmer, ms, t)
                got = engine.signature_cluster(sig, length, kmer, t, ms)
                print("kmer %d minShared %d T %g: %d representatives, %r" % (kmer, ms, t, int((want[0] == np.arange(n)).sum()), want[2]))
                same(got, want)
                strips, reps, merged, steps = engine.signature_cluster_stats()
                assert strips == 1 and reps == int((want[0] == np.arange(n)).sum()) and merged == n * n and steps == reps
                told |= {k for k in ("later", "tied", "chains") if want[2][k]}
                if want[2]["later"] and want[2]["tied"] and want[2]["chains"]:
                    told.add("together")
                rep, link = got
                assert (rep[length == 0] == np.flatnonzero(length == 0)).all()           # an empty signature is its own representative
                if t == 100.0 and length[11] >= ms:                                      # the copied row
                    assert rep[42] == first and rep[first] == first
                    assert link[42].tolist() == (first, length[11], length[11], 100.0)
    # the data tells the rules apart, all three in one parameter set
    assert told == {"later", "tied", "chains", "together"}, told


def test_definition_small_cpu_build(emu_engine, monkeypatch):
    definition_small(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_definition_small_gpu(gpu_engine, monkeypatch):
    definition_small(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the composition (rule 5)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clade_data():
    """300 genomes at size 128: 75 sets of random_sets, each followed by three copies that lose and gain values at rising rates"""
    rng = np.random.default_rng(59)
    size, universe = 128, 6000
    sets = []
    for base in random_sets(rng, 75, size, universe):
        sets.append(base)
        for rate in (0.03, 0.1, 0.25):
            kept = base[rng.random(len(base)) >= rate]
            new = rng.integers(0, universe, int(len(base) * rate)).astype(np.uint32) * np.uint32(2 ** 32 // universe - 1)
            sets.append(np.concatenate([kept, new]))
    order = rng.permutation(len(sets))                                # copies before and after what they were copied from
    return make_signatures([sets[i] for i in order], size)


def composition(engine, monkeypatch):
    sig, length = clade_data()
    n = len(sig)
    assert n == 300
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    for ms, thresholds in ((1, (90.0, 97.0)), (4, (94.0,))):
        pairs = engine.signature_pairs(sig, length, 16, ms)
        rows = np.zeros(len(pairs), dtype=CGI_DT)
        rows["refGenomeId"], rows["qryGenomeId"], rows["identity"] = pairs["a"], pairs["b"], pairs["identity"]
        cell = {(int(p["a"]), int(p["b"])): (int(p["shared"]), int(p["size"])) for p in pairs}
        for t in thresholds:
            wrep, wident = engine.cluster_greedy(rows, n, t)
            rep, link = engine.signature_cluster(sig, length, 16, t, ms)
            assert np.array_equal(rep, wrep)
            own = rep == np.arange(n)
            assert np.array_equal(link["identity"][~own].view(np.uint32), wident[~own].view(np.uint32))
            assert (link[own] == UNUSED).all() and (link["neighbor"][~own] == rep[~own]).all()
            for i in np.flatnonzero(~own):
                assert (int(link[i]["shared"]), int(link[i]["size"])) == cell[(min(i, rep[i]), max(i, rep[i]))]
            with_members = len(set(rep[~own].tolist()))
            print("minShared %d T %g: %d representatives, %d of them with members, %d members joined a later one"
                  % (ms, t, int(own.sum()), with_members, int((rep > np.arange(n)).sum())))
            assert with_members >= 20 and (rep > np.arange(n)).any()                     # tens of clusters, and the second sweep matters
            assert engine.signature_cluster_stats()[:2] == (2, int(own.sum()))           # the cap on the strip height: 256 rows below 8192 genomes


def test_composition_cpu_build(emu_engine, monkeypatch):
    composition(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_composition_gpu(gpu_engine, monkeypatch):
    composition(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. strips and shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def strips_and_shapes(engine, monkeypatch):
    """every strip height x every tile shape gives the result of case 1: height 1 makes every in-strip block 1 x 1, a height of at least n
    makes the first sweep one resolve of the whole set and the second sweep empty, and the heights between put members and their
    later representatives in different strips"""
    sig, length, cells = small_cells()
    n = len(sig)
    second = set()
    for kmer, ms, t in ((16, 1, 90.0), (16, 3, 85.0), (9, 1, 70.0)):
        want = greedy_expected(cells, n, kmer, ms, t)
        wrep = want[0]
        n_rep = int((wrep == np.arange(n)).sum())
        for strip in (None, 1, 2, 7, 16, 17, 64):
            h = n if strip is None else min(strip, n)
            # members whose representative lies in a later strip: only the second sweep finds it
            across = [i for i in range(n) if wrep[i] // h > i // h]
            if across:
                second.add(strip)
            # the launches: strip x earlier representatives, strip x strip, strip x later representatives where the strip has members
            merged, after = 0, 0
            for r0 in range(0, n, h):
                rows = min(h, n - r0)
                before, after = after, int(((wrep == np.arange(n)) & (np.arange(n) < r0 + rows)).sum())
                merged += rows * before + rows * rows + (rows * (n_rep - after) if after - before < rows else 0)
            for shape in (None, "square", "thin"):
                set_env(monkeypatch, STRIP, strip)
                set_env(monkeypatch, SHAPE, shape)
                same(engine.signature_cluster(sig, length, kmer, t, ms), want)
                stats = engine.signature_cluster_stats()
                assert stats[0] == -(-n // h) and stats[1] == n_rep, (strip, shape, stats)
                assert stats[2] == merged, (strip, shape, stats, merged)
                assert stats[3] == n_rep                                                 # every sweep of this data is one step: h <= 256
    assert second >= {1, 2, 7, 16, 17} and None not in second and 64 not in second


def test_strips_and_shapes_cpu_build(emu_engine, monkeypatch):
    strips_and_shapes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_strips_and_shapes_gpu(gpu_engine, monkeypatch):
    strips_and_shapes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pitch classes
# ---------------------------------------------------------------------------------------------------------------------------------
def pitch_classes(engine, monkeypatch):
    """40 genomes at a size of every instance of the merge tiles (pitch <= 256, <= 1024, <= 2048, above) and at sizes that are no
    multiple of four, where a staged row ends in a zeroed quad tail; the square tile of the class by the strip height, the thin tile
    forced, and ragged strips of 7 rows; against numpy alone.  Random sets at a third of their universe share a fifth of their union, an
    estimate of 93: the thresholds on both sides of it give members and several representatives."""
    rng = np.random.default_rng(61)
    for size in (16, 17, 256, 1000, 1025, 2049):
        sets = [rng.choice(3 * size, size=int(rng.integers(size * 4 // 5, size * 4 // 3)), replace=False) * (2 ** 32 // (3 * size) - 1) for _ in range(40)]
        sets[31] = sets[4]                                                               # a copy
        sets[17] = sets[17][: size // 3]                                                 # a short one
        sets[23] = sets[23][:0]                                                          # an empty one
        sig, length = make_signatures(sets, size)
        assert (length == size).any() and (0 < length).any() and (length < size).any()
        cells = cells_of(sig, length)
        members = reps = 0
        for t in (92.0, 94.0):
            want = greedy_expected(cells, 40, 16, 1, t)
            members += want[2]["members"]
            reps = max(reps, 40 - want[2]["members"])
            assert want[0][31] == want[0][4] and want[0][23] == 23
            for strip, shape in ((None, None), (None, "thin"), (7, None)):
                set_env(monkeypatch, STRIP, strip)
                set_env(monkeypatch, SHAPE, shape)
                same(engine.signature_cluster(sig, length, 16, t), want)
        assert members >= 3 and reps >= 3, (size, members, reps)


def test_pitch_classes_cpu_build(emu_engine, monkeypatch):
    pitch_classes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_pitch_classes_gpu(gpu_engine, monkeypatch):
    pitch_classes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. edges and errors
# ---------------------------------------------------------------------------------------------------------------------------------
def edges_and_errors(engine, monkeypatch):
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9], [1, 2, 3]], 3)
    lib, h = engine.lib, engine.h
    rep, link = np.full(4, -7, np.int32), np.zeros(4, dtype=NEIGHBOR_DT)
    link[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)
    stats = (ctypes.c_uint64 * 4)()

    def call(n=4, size=3, kmer=16, ms=1, mi=90.0, sig_p=sig.ctypes.data, len_p=length.ctypes.data, rep_p=rep.ctypes.data, link_p=link.ctypes.data, ctx=h):
        return lib.ani_signature_cluster(ctx, sig_p, len_p, n, size, kmer, ms, ctypes.c_float(mi), rep_p, link_p)

    # [1, 2, 3] and [2, 3, 4]: the first three of the union hold two shared values
    w = float(identity_expected(2, 3, 16))
    assert call() == 0 and rep.tolist() == [0, 0, 2, 0]
    assert link.tolist() == [(-1, 0, 0, 0.0), (0, 2, 3, w), (-1, 0, 0, 0.0), (0, 3, 3, 100.0)]
    assert lib.ani_signature_cluster_stats(h, stats) == 0 and list(stats) == [1, 2, 16, 2]
    assert call(mi=100.0) == 0 and rep.tolist() == [0, 1, 2, 0] and link[3].tolist() == (0, 3, 3, 100.0)
    assert engine.signature_cluster_stats() == (1, 3, 16, 3)
    assert lib.ani_signature_cluster_stats(h, None) == -1
    # rule 6, one case at a time
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for kmer in (0, -3, 17):
        assert call(kmer=kmer) == -1, kmer
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for mi in (0.0, -0.0, -1.0, 100.5, float("nan"), float("inf")):
        assert call(mi=mi) == -1, mi
        with pytest.raises(AniError) as ex:
            engine.signature_cluster(sig, length, 16, mi)
        assert ex.value.code == -1, mi
    assert call(n=-1) == -1
    for null in ("sig_p", "len_p", "rep_p", "link_p", "ctx"):
        assert call(**{null: None}) == -1, null
    for bad_len in ([3, 4, 1, 3], [3, -1, 1, 3]):
        with pytest.raises(AniError) as ex:
            engine.signature_cluster(sig, np.array(bad_len, dtype=np.int32), 16, 90.0)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.signature_cluster(x, length, 16, 90.0)
        assert ex.value.code == -1, bad_row
    with pytest.raises(AniError) as ex:                                # a lone row is checked too
        engine.signature_cluster(np.array([[3, 2, 1]], np.uint32), np.array([3], np.int32), 16, 90.0)
    assert ex.value.code == -1
    with pytest.raises(ValueError):
        engine.signature_cluster(sig, length[:3], 16, 90.0)
    # rule 7: the limit, before anything is read; the scalar checks before the limit
    assert call(n=(1 << 30) + 1, sig_p=None, len_p=None, rep_p=None, link_p=None) == -4
    tiny = np.zeros(1, np.uint32)
    assert call(n=(1 << 30) + 1, sig_p=tiny.ctypes.data, len_p=tiny.ctypes.data) == -4
    assert call(n=(1 << 30) + 1, mi=0.0) == -1 and call(n=(1 << 30) + 1, size=0) == -1
    # rule 8: no genomes
    rep[:], link[:] = -7, np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)
    assert call(n=0) == 0 and call(n=0, sig_p=None, len_p=None, rep_p=None, link_p=None) == 0
    assert (rep == -7).all() and (link["neighbor"] == -7).all()
    assert engine.signature_cluster_stats() == (0, 0, 0, 0)
    assert call(n=0, mi=0.0) == -1 and call(n=0, ms=0) == -1
    r0, l0 = engine.signature_cluster(sig[:0], length[:0], 16, 90.0)
    assert r0.shape == (0,) and r0.dtype == np.int32 and l0.shape == (0,) and l0.dtype == NEIGHBOR_DT
    # one genome, empty or not
    for row in ([5, 6, 7], []):
        s1, l1 = make_signatures([row], 3)
        r1, k1 = engine.signature_cluster(s1, l1, 16, 50.0)
        assert r1.tolist() == [0] and (k1 == UNUSED).all()
        assert engine.signature_cluster_stats() == (1, 1, 1, 1)
    for strip in (None, 3):
        set_env(monkeypatch, STRIP, strip)
        # all signatures empty: every genome is its own representative
        se, le = make_signatures([[]] * 9, 5)
        re_, ke = engine.signature_cluster(se, le, 16, 1.0)
        assert re_.tolist() == list(range(9)) and (ke == UNUSED).all()
        # all signatures identical: one representative, everyone else at exactly 100
        si, li = make_signatures([[4, 8, 15, 16]] * 9, 5)
        ri, ki = engine.signature_cluster(si, li, 16, 100.0, 4)
        assert ri.tolist() == [0] * 9 and (ki[0] == UNUSED) and ki[1:].tolist() == [(0, 4, 4, 100.0)] * 8
        assert engine.signature_cluster_stats()[:2] == (1 if strip is None else 3, 1)
        rj, kj = engine.signature_cluster(si, li, 16, 100.0, 5)                          # ... unless they share too little
        assert rj.tolist() == list(range(9)) and (kj == UNUSED).all()


def test_edges_and_errors_cpu_build(emu_engine, monkeypatch):
    edges_and_errors(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_edges_and_errors_gpu(gpu_engine, monkeypatch):
    edges_and_errors(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cli(binary, engine, tmp, n_len):
    lst, paths, genomes = two_genera(tmp, n_len)
    size, t = 200, 90.0
    sk = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes)
    sig, length = sk.signatures(size)
    sk.close()
    rep, link = engine.signature_cluster(sig, length, 16, t)
    same((rep, link), greedy_expected(cells_of(sig, length), len(paths), 16, 1, t))      # the API's answer is the restatement's
    want = "".join("%s\t%s\t%s\n" % (paths[g], paths[rep[g]], "NA\tNA" if rep[g] == g else "%s\t%d/%d" % ("%g" % link[g]["identity"], link[g]["shared"], link[g]["size"]))
                   for g in range(len(paths)))
    assert rep.tolist() == [0, 0, 0, 3, 3, 3]                          # the two genera, each around its first genome

    common = ["--ql", lst, "--rl", lst, "--matrix"]
    base, out = os.path.join(tmp, "base.out"), os.path.join(tmp, "cl.out")
    assert run(binary, common + ["-o", base]).returncode == 0
    r = run(binary, common + ["--sketchCluster", "90", "--sketchSize", str(size), "-o", out], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"sketch clusters found" in r.stderr and b"sketch clusters written" in r.stderr and b"sketch pairs compared" not in r.stderr
    assert open(out + ".sketchclusters").read() == want
    # without the option every file is as before; with it, every other file
    assert not os.path.exists(base + ".sketchclusters")
    made = sorted(f[len("cl.out"):] for f in os.listdir(tmp) if f.startswith("cl.out"))
    assert made == ["", ".matrix", ".sketchclusters"] and sorted(f[len("base.out"):] for f in os.listdir(tmp) if f.startswith("base.out")) == ["", ".matrix"]
    for ext in ("", ".matrix"):
        assert open(out + ext, "rb").read() == open(base + ext, "rb").read(), ext
    # a forced strip height of 3: the same file
    o3 = os.path.join(tmp, "strip3.out")
    r = run(binary, common + ["--sketchCluster", "90", "--sketchSize", str(size), "-o", o3], {STRIP: "3"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(o3 + ".sketchclusters").read() == want
    # refused by name: the threshold, and a query that is no reference, before anything is mapped
    bad = os.path.join(tmp, "bad.out")
    for value in ("0", "101", "-3", "x"):
        r = run(binary, common + ["--sketchCluster", value, "-o", bad])
        assert r.returncode == 1 and b"ERROR, --sketchCluster takes an ANI threshold in (0, 100]" in r.stderr, (value, r.stderr[-300:])
    rl = os.path.join(tmp, "r.txt")
    open(rl, "w").write("".join(p + "\n" for p in paths[:4] + paths[5:]))
    r = run(binary, ["--ql", lst, "--rl", rl, "--sketchCluster", "90", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"--sketchCluster" in r.stderr and b"is not among the references" in r.stderr and paths[4].encode() in r.stderr, r.stderr[-500:]
    assert b"devices initialised" not in r.stderr and b"queries mapped" not in r.stderr
    assert not os.path.exists(bad) and not os.path.exists(bad + ".sketchclusters")
    assert b"--sketchCluster" in run(binary, ["-h"]).stdout


def test_cli_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 8000)


@pytest.mark.gpu
def test_cli_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
