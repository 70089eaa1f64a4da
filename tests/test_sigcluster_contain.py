"""Greedy representative clustering under the containment estimate (ani_signature_cluster_contain, Engine.signature_cluster_contain,
fastANI --sketchCluster T --sketchContain max) against a plain-Python restatement: the greedy rule of test_sigcluster (rules 2 - 4 of
ani_signature_cluster) over the numpy cells of test_sigcontain (rules 1 - 5 of ani_signature_screen_contain) in mode max, and against
the composition the header names: engine.cluster_greedy over the rows of engine.signature_graph(estimate="contain").  Everything is
integer or one host pow, so every comparison is exact: ids, shared, denominator, identity by bit pattern, and the unused record of a
representative.  The expected values never come from the call under test.  CPU: the tests/emu build of the library and of the command
line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import fastani_amd
import orc
import test_sigcluster
from fastani_amd.api import CGI_DT, NEIGHBOR_DT, AniError
from test_sigcluster import UNUSED, clade_data, same
from test_sigcontain import MAX, cell_expected, denominator, identity_expected
from test_sigdist import make_signatures, pair_expected, random_sets, two_genera
from test_sigdist import identity_expected as mash_identity_expected
from test_sigscreen import EMU, ROOT, SHAPE, STRIP, bits, run, set_env, small_data

TRI = "ANI_TEST_SIG_CLUSTER_TRI"


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def cells_of(sig, length):
    """the pair of the header: (shared, d) of every a < b, Q the signature of a and R that of b, d = min(inQ, inR)"""
    n, size = sig.shape
    out = {}
    for a in range(n):
        for b in range(a + 1, n):
            cell = cell_expected(sig[a, :length[a]], sig[b, :length[b]], size)
            out[(a, b)] = (cell[0], denominator(cell, MAX))
    return out


def greedy_expected(cells, n, kmer, min_shared, min_identity):
    """the greedy rule of test_sigcluster as it stands, reading the identity of a cell from rule 5 of the containment estimate
    instead of the Mash one -> (representative, link, facts)"""
    mash = test_sigcluster.identity_of
    test_sigcluster.identity_of = identity_expected
    try:
        return test_sigcluster.greedy_expected(cells, n, kmer, min_shared, min_identity)
    finally:
        test_sigcluster.identity_of = mash


def representatives(rep):
    return int((rep == np.arange(len(rep))).sum())


def launches(wrep, n, h, tri):
    """cells the launches of a call walk: strip x earlier representatives, the strip's own block (rows (rows - 1) / 2 from its upper
    triangle, rows^2 in full), strip x later representatives where the strip has members; and the sum of rows (rows + 1) / 2"""
    is_rep = wrep == np.arange(n)
    n_rep = int(is_rep.sum())
    merged = after = saved = 0
    for r0 in range(0, n, h):
        rows = min(h, n - r0)
        before, after = after, int(is_rep[:r0 + rows].sum())
        merged += rows * before + (rows * (rows - 1) // 2 if tri else rows * rows) + (rows * (n_rep - after) if after - before < rows else 0)
        saved += rows * (rows + 1) // 2
    return merged, saved


@functools.lru_cache(maxsize=None)
def small_cells():
    sig, length = small_data()
    return sig, length, cells_of(sig, length)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the definition on the small set
# ---------------------------------------------------------------------------------------------------------------------------------
def definition_small(engine, monkeypatch):
    """63 sets of size 16 from a small pool, lengths 0 to 16: empty rows, truncated rows (length 16) and whole ones"""
    sig, length, cells = small_cells()
    n = len(sig)
    assert (length == 0).any() and (length == 16).any() and ((0 < length) & (length < 16)).any()
    for name in (STRIP, SHAPE, TRI):
        set_env(monkeypatch, name, None)
    # the cells are not those of the Mash merge: the two calls answer different questions on this data
    assert any(cells[a, b] != pair_expected(sig[a, :length[a]], sig[b, :length[b]], 16) for a, b in cells)
    first = min(r for r in range(n) if length[r] == length[11] and (sig[r] == sig[11]).all())
    for kmer, ms in ((16, 1), (16, 3), (9, 1)):
        for t in (90.0, 95.0, 97.0):
            want = greedy_expected(cells, n, kmer, ms, t)
            got = engine.signature_cluster_contain(sig, length, kmer, t, "max", ms)
            print("kmer %d minShared %d T %g: %d representatives, %r" % (kmer, ms, t, representatives(want[0]), want[2]))
            same(got, want)
            assert engine.signature_cluster_stats() == (1, representatives(want[0]), n * (n - 1) // 2, representatives(want[0]))
            same(engine.signature_cluster_contain(sig, length, kmer, t, 2, ms), want)       # the mode by number; the default is "max"
            same(engine.signature_cluster_contain(sig, length, kmer, t, min_shared=ms), want)
            if kmer == 16:
                # a member whose representative has the larger id, and a tie between two representatives that goes to the smaller id
                assert want[2]["later"] >= 1 and want[2]["tied"] >= 1 and want[2]["members"] >= 20, want[2]
            rep, link = got
            assert (rep[length == 0] == np.flatnonzero(length == 0)).all()                   # an empty signature is its own representative
            if length[11] >= ms:                                                             # the copied row joins where its original is
                assert rep[42] == rep[first]
                if rep[first] == first:
                    assert link[42].tolist() == (first, length[11], length[11], 100.0)


def test_definition_small_cpu_build(emu_engine, monkeypatch):
    definition_small(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_definition_small_gpu(gpu_engine, monkeypatch):
    definition_small(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. partial genomes: what the call is for
# ---------------------------------------------------------------------------------------------------------------------------------
PARTIAL_T = 99.0


@functools.lru_cache(maxsize=None)
def partial_data():
    """8 species at size 32.  A species is 60 values of a range of its own, so its signature is truncated (its 32 smallest); its two
    partial copies hold a random half (30) and a random 40 % (24) of the 60 values and are not.  The parents are genomes 0 .. 7, the
    copies follow in a random order.  -> sig, length, parent of every genome"""
    rng = np.random.default_rng(67)
    size, sets, parent = 32, [], []
    species = [np.sort(rng.choice(10 ** 6, size=60, replace=False)) + s * 10 ** 7 for s in range(8)]
    parts = [(s, rng.choice(species[s], size=m, replace=False)) for s in range(8) for m in (30, 24)]
    for s in range(8):
        sets.append(species[s])
        parent.append(s)
    for i in rng.permutation(len(parts)):
        sets.append(parts[i][1])
        parent.append(parts[i][0])
    sig, length = make_signatures(sets, size)
    assert (length[:8] == size).all() and sorted(length[8:].tolist()) == [24] * 8 + [30] * 8
    return sig, length, np.array(parent)


def partial_genomes(engine, monkeypatch):
    """The Jaccard estimate of a half against its whole is shared / size = 1 / 2 or so, 97.5 at kmerSize 16, and 96.5 for 40 %: below
    the threshold of 99, where every partial copy is a representative of its own.  The containment estimate divides by the part of
    the copy inside the parent's range, all of which is shared: 100."""
    sig, length, parent = partial_data()
    n, size = sig.shape
    for name in (STRIP, SHAPE, TRI):
        set_env(monkeypatch, name, None)
    # the inputs, by the restatements alone
    for g in range(8, n):
        p = int(parent[g])
        q, r = sig[p, :length[p]], sig[g, :length[g]]
        sh, sz = pair_expected(q, r, size)
        mash = mash_identity_expected(sh, sz, 16)
        cell = cell_expected(q, r, size)
        contain = identity_expected(cell[0], denominator(cell, MAX), 16)
        assert 0 < mash < PARTIAL_T <= contain == 100.0, (g, sh, sz, cell)
    for a in range(8):                                                                       # species share nothing
        for b in range(a + 1, 8):
            assert cell_expected(sig[a], sig[b], size)[0] == 0
    rep, link = engine.signature_cluster_contain(sig, length, 16, PARTIAL_T)
    assert np.array_equal(rep, parent.astype(np.int32)) and representatives(rep) == 8
    assert (link["identity"][8:] == 100.0).all() and (link["shared"][8:] == link["size"][8:]).all() and (link[:8] == UNUSED).all()
    mrep, _ = engine.signature_cluster(sig, length, 16, PARTIAL_T)
    assert representatives(mrep) == n > 8                                                    # the Mash call leaves every copy alone
    same((rep, link), greedy_expected(cells_of(sig, length), n, 16, 1, PARTIAL_T))


def test_partial_genomes_cpu_build(emu_engine, monkeypatch):
    partial_genomes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_partial_genomes_gpu(gpu_engine, monkeypatch):
    partial_genomes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the composition
# ---------------------------------------------------------------------------------------------------------------------------------
def composition(engine, monkeypatch):
    """the 300 genomes in clades of test_sigcluster: the call is cluster_greedy over the records of the containment graph"""
    sig, length = clade_data()
    n = len(sig)
    assert n == 300
    for name in (STRIP, SHAPE, TRI):
        set_env(monkeypatch, name, None)
    for ms, thresholds in ((1, (92.0, 97.0)), (4, (95.0,))):
        pairs = engine.signature_graph(sig, length, 16, 0.0, ms, "contain")
        assert (pairs["shared"] >= ms).all()
        rows = np.zeros(len(pairs), dtype=CGI_DT)
        rows["refGenomeId"], rows["qryGenomeId"], rows["identity"] = pairs["a"], pairs["b"], pairs["identity"]
        cell = {(int(p["a"]), int(p["b"])): (int(p["shared"]), int(p["size"])) for p in pairs}
        for t in thresholds:
            wrep, wident = engine.cluster_greedy(rows, n, t)
            rep, link = engine.signature_cluster_contain(sig, length, 16, t, "max", ms)
            assert np.array_equal(rep, wrep)
            own = rep == np.arange(n)
            assert np.array_equal(link["identity"][~own].view(np.uint32), wident[~own].view(np.uint32))
            assert (link[own] == UNUSED).all() and (link["neighbor"][~own] == rep[~own]).all()
            for i in np.flatnonzero(~own):
                assert (int(link[i]["shared"]), int(link[i]["size"])) == cell[(min(i, rep[i]), max(i, rep[i]))]
            with_members = len(set(rep[~own].tolist()))
            print("minShared %d T %g: %d representatives, %d of them with members, %d members joined a later one"
                  % (ms, t, int(own.sum()), with_members, int((rep > np.arange(n)).sum())))
            assert with_members >= 20 and (rep > np.arange(n)).any()                         # tens of clusters, and the second sweep matters
            assert engine.signature_cluster_stats()[:2] == (2, int(own.sum()))


def test_composition_cpu_build(emu_engine, monkeypatch):
    composition(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_composition_gpu(gpu_engine, monkeypatch):
    composition(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. strips, shapes and the triangle
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip_data():
    """150 related sets at size 32 (a walk is at most 64 steps), and what the rules make of them"""
    sig, length = make_signatures(random_sets(np.random.default_rng(71), 150, 32, 400), 32)
    assert (length == 32).any() and (length == 0).any()
    return sig, length, greedy_expected(cells_of(sig, length), 150, 16, 1, 95.0)


def strips_and_shapes(engine, monkeypatch):
    """every strip height x every tile shape x the triangular block or the full one: one result.  Heights 1, 3 and 7 make a diagonal
    tile that is partly empty, 64 leaves a ragged last strip of 22 rows with tiles right of the diagonal, 150 is the whole set in one
    block of 10 x 10 tiles, 4096 is clamped to it.  The two settings of the triangle differ by rows (rows + 1) / 2 walked cells per
    strip and in nothing else."""
    sig, length, want = strip_data()
    n = len(sig)
    wrep = want[0]
    assert 10 <= representatives(wrep) <= 100 and want[2]["later"] >= 1, want[2]
    second = set()
    for strip in (1, 3, 7, 64, 150, 4096):
        h = min(strip, n)
        if any(wrep[i] // h > i // h for i in range(n)):
            second.add(strip)
        for shape in (None, "square", "thin"):
            stats = {}
            for tri in (None, 0):
                set_env(monkeypatch, STRIP, strip)
                set_env(monkeypatch, SHAPE, shape)
                set_env(monkeypatch, TRI, tri)
                same(engine.signature_cluster_contain(sig, length, 16, 95.0), want)
                stats[tri] = engine.signature_cluster_stats()
                merged, saved = launches(wrep, n, h, tri is None)
                assert stats[tri][:3] == (-(-n // h), representatives(wrep), merged), (strip, shape, tri, stats[tri], merged)
            assert stats[0][2] - stats[None][2] == saved and stats[0][3] == stats[None][3], (strip, shape, stats)
    assert second >= {1, 3, 7} and not second & {150, 4096}                                  # the second sweep had members to place


def test_strips_and_shapes_cpu_build(emu_engine, monkeypatch):
    strips_and_shapes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_strips_and_shapes_gpu(gpu_engine, monkeypatch):
    strips_and_shapes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pitch classes
# ---------------------------------------------------------------------------------------------------------------------------------
PITCH_CASES = ((3, 40), (10, 40), (16, 40), (250, 40), (1000, 36), (1500, 28), (2048, 24), (4096, 20))      # size, genomes


def pitch_classes(engine, monkeypatch, size, n):
    """A size of every instance of the merge tiles (pitch <= 256, <= 1024, <= 2048, above), sizes that are no multiple of four, where a
    staged row ends in a zeroed quad tail, and rows of an even (1000, 2048, 4096) and an odd (250, 1500) number of quads, which decides
    the pitch of a row in LDS; more genomes than a tile has rows, so that tiles right of the diagonal run; against numpy alone, the
    triangle both ways, and ragged strips of 7 rows.  Random sets at a third of their universe share a third of either: an estimate of
    93.4 to 94, ever closer to it as the size grows: a threshold below it makes nearly every genome a member, one above it nearly every
    genome a representative, and one inside the range gives both where the size is small."""
    rng = np.random.default_rng(73 + size)
    universe = 3 * size + 6
    sets = [rng.choice(universe, size=int(rng.integers(size * 4 // 5, size * 4 // 3 + 2)), replace=False) * (2 ** 32 // universe - 1) for _ in range(n)]
    sets[n - 1] = sets[4]                                                                    # a copy
    sets[17] = np.sort(sets[2])[: max(1, size // 3)]                                         # a part of another: all of it is shared
    sets[11] = sets[11][:0]                                                                  # an empty one
    sig, length = make_signatures(sets, size)
    assert (length == size).any() and (0 < length).any() and (length < size).any()
    cells = cells_of(sig, length)
    assert cells[(2, 17)] == (length[17], length[17]) and 0 < length[17] < length[2]
    members = reps = 0
    for t in (92.0, 94.0, 95.0):
        want = greedy_expected(cells, n, 16, 1, t)
        members += want[2]["members"]
        reps = max(reps, n - want[2]["members"])
        assert want[0][n - 1] == want[0][4] and want[0][11] == 11
        for strip, shape in ((None, None), (None, "thin"), (7, None)):
            for tri in (None, 0):
                set_env(monkeypatch, STRIP, strip)
                set_env(monkeypatch, SHAPE, shape)
                set_env(monkeypatch, TRI, tri)
                same(engine.signature_cluster_contain(sig, length, 16, t), want)
    assert members >= 3 and reps >= 3, (size, members, reps)


@pytest.mark.parametrize("size,n", PITCH_CASES)
def test_pitch_classes_cpu_build(emu_engine, monkeypatch, size, n):
    pitch_classes(emu_engine, monkeypatch, size, n)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n", PITCH_CASES)
def test_pitch_classes_gpu(gpu_engine, monkeypatch, size, n):
    pitch_classes(gpu_engine, monkeypatch, size, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. arguments and edges
# ---------------------------------------------------------------------------------------------------------------------------------
def arguments(engine, monkeypatch):
    for name in (STRIP, SHAPE, TRI):
        set_env(monkeypatch, name, None)
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9], [1, 2, 3], [2, 3]], 3)
    lib, h = engine.lib, engine.h
    rep, link = np.full(5, -7, np.int32), np.zeros(5, dtype=NEIGHBOR_DT)
    link[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)
    stats = (ctypes.c_uint64 * 4)()

    def call(n=5, size=3, kmer=16, ms=1, mi=90.0, mode=2, sig_p=sig.ctypes.data, len_p=length.ctypes.data, rep_p=rep.ctypes.data, link_p=link.ctypes.data, ctx=h):
        return lib.ani_signature_cluster_contain(ctx, sig_p, len_p, n, size, kmer, ms, ctypes.c_float(mi), mode, rep_p, link_p)

    mash_before = engine.signature_cluster(sig, length, 16, 90.0)
    # [1, 2, 3] and [2, 3, 4], both truncated: 2 and 3 are shared; of the first, 1, 2, 3 are <= 4; of the second, 2, 3 are <= 3: d = 2.
    # [2, 3] is whole, so all of it counts, and all of it is in either.
    assert call() == 0 and rep.tolist() == [0, 0, 2, 0, 0]
    assert link.tolist() == [(-1, 0, 0, 0.0), (0, 2, 2, 100.0), (-1, 0, 0, 0.0), (0, 3, 3, 100.0), (0, 2, 2, 100.0)]
    assert lib.ani_signature_cluster_stats(h, stats) == 0 and list(stats) == [1, 2, 10, 2]
    # the Mash call on the same rows, before and after: what it returned before, and its own stats
    mash = engine.signature_cluster(sig, length, 16, 90.0)
    same(mash, mash_before)
    assert mash[1][1].tolist() == (0, 2, 3, float(mash_identity_expected(2, 3, 16))) and engine.signature_cluster_stats() == (1, 2, 25, 2)
    # minShared larger than every shared: nobody has an edge
    assert call(ms=4) == 0 and rep.tolist() == [0, 1, 2, 3, 4] and (link == UNUSED).all()
    assert engine.signature_cluster_stats() == (1, 5, 10, 5)
    # the mode: only the symmetric one, and the message says why
    for mode in (0, 1, 3, -1):
        assert call(mode=mode) == -1, mode
        with pytest.raises(AniError) as ex:
            engine.signature_cluster_contain(sig, length, 16, 90.0, mode)
        assert ex.value.code == -1
        if mode in (0, 1):
            assert "symmetric" in str(ex.value)
    for name in ("query", "reference"):
        with pytest.raises(AniError) as ex:
            engine.signature_cluster_contain(sig, length, 16, 90.0, name)
        assert ex.value.code == -1 and "symmetric" in str(ex.value)
    for name in ("Max", "jaccard", ""):
        with pytest.raises(ValueError):
            engine.signature_cluster_contain(sig, length, 16, 90.0, name)
    # rule 6 of ani_signature_cluster, one case at a time
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for kmer in (0, -3, 17):
        assert call(kmer=kmer) == -1, kmer
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for mi in (0.0, -0.0, -1.0, 100.0001, 100.5, float("nan"), float("inf")):
        assert call(mi=mi) == -1, mi
        with pytest.raises(AniError) as ex:
            engine.signature_cluster_contain(sig, length, 16, mi)
        assert ex.value.code == -1, mi
    assert call(mi=100.0) == 0 and rep.tolist() == [0, 0, 2, 0, 0]                           # (100 itself is inside)
    assert call(n=-1) == -1
    for null in ("sig_p", "len_p", "rep_p", "link_p", "ctx"):
        assert call(**{null: None}) == -1, null
    for bad_len in ([3, 4, 1, 3, 2], [3, -1, 1, 3, 2]):
        with pytest.raises(AniError) as ex:
            engine.signature_cluster_contain(sig, np.array(bad_len, dtype=np.int32), 16, 90.0)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.signature_cluster_contain(x, length, 16, 90.0)
        assert ex.value.code == -1, bad_row
    with pytest.raises(AniError) as ex:                                # a lone row is checked too
        engine.signature_cluster_contain(np.array([[3, 2, 1]], np.uint32), np.array([3], np.int32), 16, 90.0)
    assert ex.value.code == -1
    with pytest.raises(ValueError):
        engine.signature_cluster_contain(sig, length[:3], 16, 90.0)
    # the limit, before anything is read; the scalar checks, the mode among them, before the limit
    assert call(n=(1 << 30) + 1, sig_p=None, len_p=None, rep_p=None, link_p=None) == -4
    assert call(n=(1 << 30) + 1, mi=0.0) == -1 and call(n=(1 << 30) + 1, size=0) == -1 and call(n=(1 << 30) + 1, mode=0) == -1
    # no genomes
    rep[:], link[:] = -7, np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)
    assert call(n=0) == 0 and call(n=0, sig_p=None, len_p=None, rep_p=None, link_p=None) == 0
    assert (rep == -7).all() and (link["neighbor"] == -7).all()
    assert engine.signature_cluster_stats() == (0, 0, 0, 0)
    assert call(n=0, mi=0.0) == -1 and call(n=0, ms=0) == -1 and call(n=0, mode=1) == -1 and call(n=0, mode=3) == -1
    r0, l0 = engine.signature_cluster_contain(sig[:0], length[:0], 16, 90.0)
    assert r0.shape == (0,) and r0.dtype == np.int32 and l0.shape == (0,) and l0.dtype == NEIGHBOR_DT
    # one genome, empty or not: a block of one row has no pair to walk
    for row in ([5, 6, 7], []):
        s1, l1 = make_signatures([row], 3)
        r1, k1 = engine.signature_cluster_contain(s1, l1, 16, 50.0)
        assert r1.tolist() == [0] and (k1 == UNUSED).all()
        assert engine.signature_cluster_stats() == (1, 1, 0, 1)
    for strip in (None, 3):
        for tri in (None, 0):
            set_env(monkeypatch, STRIP, strip)
            set_env(monkeypatch, TRI, tri)
            # all signatures empty: every genome is its own representative
            se, le = make_signatures([[]] * 9, 5)
            re_, ke = engine.signature_cluster_contain(se, le, 16, 1.0)
            assert re_.tolist() == list(range(9)) and (ke == UNUSED).all()
            # all signatures identical: one representative, everyone else at exactly 100
            si, li = make_signatures([[4, 8, 15, 16]] * 9, 5)
            ri, ki = engine.signature_cluster_contain(si, li, 16, 100.0, "max", 4)
            assert ri.tolist() == [0] * 9 and (ki[0] == UNUSED) and ki[1:].tolist() == [(0, 4, 4, 100.0)] * 8
            assert engine.signature_cluster_stats()[:2] == (1 if strip is None else 3, 1)
            rj, kj = engine.signature_cluster_contain(si, li, 16, 100.0, "max", 5)         # ... unless they share too little
            assert rj.tolist() == list(range(9)) and (kj == UNUSED).all()


def test_arguments_cpu_build(emu_engine, monkeypatch):
    arguments(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_arguments_gpu(gpu_engine, monkeypatch):
    arguments(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def clusters_text(paths, rep, link):
    return "".join("%s\t%s\t%s\n" % (paths[g], paths[rep[g]], "NA\tNA" if rep[g] == g else "%s\t%d/%d" % ("%g" % link[g]["identity"], link[g]["shared"], link[g]["size"]))
                   for g in range(len(paths)))


def run_cli(binary, engine, tmp, n_len):
    """the two genera of test_sigdist and the first half of genome 0 as a genome of its own"""
    lst, paths, genomes = two_genera(tmp, n_len)
    half = genomes[0][0][: n_len // 2]
    paths.append(os.path.join(tmp, "half.fa"))
    orc.write_fasta(paths[-1], [half], names=["half"])
    genomes.append([half])
    open(lst, "w").write("\n".join(paths) + "\n")
    size, t = 200, 90.0
    sk = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes)
    sig, length = sk.signatures(size)
    sk.close()
    assert (length == size).all()                                      # every sketch is truncated, the half's too
    rep, link = engine.signature_cluster_contain(sig, length, 16, t)
    same((rep, link), greedy_expected(cells_of(sig, length), len(paths), 16, 1, t))          # the API's answer is the restatement's
    assert rep.tolist() == [0, 0, 0, 3, 3, 3, 0]                       # the two genera, and the half with its whole
    mrep, mlink = engine.signature_cluster(sig, length, 16, t)
    # the half shares about half of the whole's sketch; all of what lies in the whole's range is shared
    assert 0 < link[6]["size"] < size and mlink[6]["size"] == size and link[6]["identity"] > mlink[6]["identity"] and link[6]["identity"] > 99.0

    common = ["--ql", lst, "--rl", lst, "--sketchCluster", "90", "--sketchSize", str(size)]
    plain, out = os.path.join(tmp, "plain.out"), os.path.join(tmp, "contain.out")
    r = run(binary, common + ["--sketchContain", "max", "-o", out], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"sketch clusters found" in r.stderr and b"sketch clusters written" in r.stderr
    text = open(out + ".sketchclusters").read()
    assert text == clusters_text(paths, rep, link)
    last = text.splitlines()[6].split("\t")
    assert last[:2] == [paths[6], paths[0]] and last[3] == "%d/%d" % (link[6]["shared"], link[6]["size"])   # shared/denominator
    # without the option: the file of the Mash call, in the format it always had, and every other file the same
    assert run(binary, common + ["-o", plain]).returncode == 0
    assert open(plain + ".sketchclusters").read() == clusters_text(paths, mrep, mlink) != text
    assert open(plain, "rb").read() == open(out, "rb").read()
    assert sorted(f[len("contain.out"):] for f in os.listdir(tmp) if f.startswith("contain.out")) == ["", ".sketchclusters"]
    # refused by name, with exit status 1, before anything is mapped
    bad = os.path.join(tmp, "bad.out")
    for mode in ("query", "reference"):
        for more in ([], ["--sketchScreen", "3"], ["--sketchGraph", "95"]):
            r = run(binary, common + more + ["--sketchContain", mode, "-o", bad], {"ANI_CLI_TRACE": "1"})
            message = b"ERROR, --sketchGraph takes --sketchContain max only" if more[:1] == ["--sketchGraph"] else b"ERROR, --sketchCluster takes --sketchContain max only"
            assert r.returncode == 1 and message in r.stderr and b"devices initialised" not in r.stderr, (mode, more, r.stderr[-300:])
    r = run(binary, ["--ql", lst, "--rl", lst, "--sketchContain", "max", "-o", bad])
    assert r.returncode == 1 and b"ERROR, --sketchContain needs --sketchScreen" in r.stderr, r.stderr[-300:]
    assert not os.path.exists(bad) and not os.path.exists(bad + ".sketchclusters")
    usage = run(binary, ["-h"]).stdout
    assert b"--sketchCluster" in usage and b"--sketchContain max" in usage


def test_cli_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 8000)


@pytest.mark.gpu
def test_cli_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
