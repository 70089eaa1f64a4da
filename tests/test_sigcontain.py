"""Sketch screening under the containment estimate (ani_signature_screen_contain, Engine.signature_screen_contain, fastANI --sketchScreen K
--sketchContain MODE) against a numpy restatement of its rules 1 - 6 (include/ani_abi.h) written here: np.intersect1d for shared,
np.searchsorted(side="right") for the parts of either list below the other's last value, math.pow on Python floats for the identity.
Every comparison is exact: ids, counts, shared, denominator, identity by bit pattern, and the unused slots.  The expected lists never
come from the call under test.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library
and fastani_amd/fastANI."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import fastani_amd
import orc
from fastani_amd.api import NEIGHBOR_DT, AniError
from test_sigdist import make_signatures, pair_expected, two_genera
from test_sigscreen import EMU, ROOT, SHAPE, STRIP, STRIPS, UNUSED, bits, lists_of, run, same, set_env, small_data, strips_of

QUERY, REF, MAX = 0, 1, 2
MODES = (QUERY, REF, MAX)


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def cell_expected(q, r, size):
    """rules 1 - 3 for a query list and a reference list (ascending, distinct) -> (shared, inQ, inR)"""
    shared = len(np.intersect1d(q, r, assume_unique=True))
    in_q = int(np.searchsorted(q, r[-1], side="right")) if len(r) == size else len(q)
    in_r = int(np.searchsorted(r, q[-1], side="right")) if len(q) == size else len(r)
    assert shared <= in_q <= size and shared <= in_r <= size
    return shared, in_q, in_r


def denominator(cell, mode):
    """rule 4"""
    _, in_q, in_r = cell
    return in_q if mode == QUERY else in_r if mode == REF else min(in_q, in_r)


@functools.lru_cache(maxsize=None)
def identity_expected(shared, d, kmer):
    """rule 5: one double expression from the exact integers, rounded once to float"""
    if shared == 0:
        return np.float32(0.0)
    return np.float32(min(max(100.0 * math.pow(float(shared) / float(d), 1.0 / float(kmer)), 0.0), 100.0))


def cells_of(ref, ref_len, qry, qry_len):
    """(shared, inQ, inR) of every (query, reference)"""
    size = ref.shape[1]
    return [[cell_expected(qry[q, :qry_len[q]], ref[r, :ref_len[r]], size) for r in range(len(ref))] for q in range(len(qry))]


def expected(cells, n_ref, n_qry, kmer, k, mode, min_shared, min_identity):
    """rule 6 over the cells of the queries [0, n_qry) and the references [0, n_ref) -> (neighbors, count), candidates per query"""
    low = bits(0.0 if min_identity == 0 else min_identity)
    cand = {}
    for q in range(n_qry):
        for r in range(n_ref):
            sh, d = cells[q][r][0], denominator(cells[q][r], mode)
            w = identity_expected(sh, d, kmer)
            if sh >= min_shared and bits(w) >= low:
                cand.setdefault(q, []).append((r, sh, d, w))
    return lists_of(cand, n_qry, k), [len(cand.get(q, [])) for q in range(n_qry)]


def record(got, q, r):
    """the record of reference r in the list of query q, or None"""
    nb, count = got
    hit = [x for x in nb[q, :count[q]] if x["neighbor"] == r]
    assert len(hit) <= 1
    return (int(hit[0]["shared"]), int(hit[0]["size"]), bits(hit[0]["identity"])) if hit else None


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the definition on the small sets
# ---------------------------------------------------------------------------------------------------------------------------------
def definition_small(engine, monkeypatch):
    sig, length = small_data()
    n_ref, n_qry = 40, 23
    ref, ref_len, qry, qry_len = sig[:n_ref], length[:n_ref], sig[n_ref:], length[n_ref:]
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    cells = cells_of(ref, ref_len, qry, qry_len)
    # the data tells the two rules apart: some pair's (shared, denominator) is not the (shared, size) of the Mash merge
    mash = [[pair_expected(ref[r, :ref_len[r]], qry[q, :qry_len[q]], 16) for r in range(n_ref)] for q in range(n_qry)]
    for mode in MODES:
        assert any((cells[q][r][0], denominator(cells[q][r], mode)) != mash[q][r] for q in range(n_qry) for r in range(n_ref)), mode
    assert any(cells[q][r][0] != mash[q][r][0] for q in range(n_qry) for r in range(n_ref))         # shared itself: not cut at 16 union elements
    fewer = more = False
    for mode in MODES:
        for kmer, idents in ((16, (0.0, 70.0, 100.0, -0.0)), (9, (0.0, 70.0))):
            for ms in (1, 3):
                for k in (1, 3, 8, 39, 64):
                    for mi in idents:
                        want, cands = expected(cells, n_ref, n_qry, kmer, k, mode, ms, mi)
                        got = engine.signature_screen_contain(ref, ref_len, qry, qry_len, kmer, k, mode, ms, mi)
                        same(got, want)
                        assert engine.signature_screen_strips() == 1
                        fewer |= any(c < k for c in cands)
                        more |= any(c > k for c in cands)
                        if mi <= 0 and length[11] >= ms:              # the copied row: at 100, in the list unless k cut a run of 100s before it
                            nb, count = got
                            assert count[2] >= 1 and bits(nb[2, 0]["identity"]) == bits(100.0)
                            assert record(got, 2, 11) == (length[11], length[11], bits(100.0)) or count[2] == k
                        assert got[1][7] == 0                         # the empty query
    assert fewer and more


def test_definition_small_cpu_build(emu_engine, monkeypatch):
    definition_small(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_definition_small_gpu(gpu_engine, monkeypatch):
    definition_small(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. directed rows
# ---------------------------------------------------------------------------------------------------------------------------------
def directed_rows(engine, monkeypatch):
    top = 0xffffffff
    set_env(monkeypatch, STRIP, None)
    for size in (16, 17):
        full = np.arange(1, size + 1) * 10                                       # truncated: `size` values, the last 10 size
        refs = [full,                                                            # 0  truncated
                np.arange(1, size + 1),                                          # 1  truncated, all below 1000
                [2, 4, 6, 8],                                                    # 2  untruncated
                [0, 2, 5, 2 * size + 10],                                        # 3  untruncated, first value 0
                np.arange(size) * 2,                                             # 4  truncated, first value 0, last 2 size - 2
                np.concatenate([np.arange(size - 1) * 3 + 1, [5000]]),           # 5  truncated, last 5000
                [0, 7, top],                                                     # 6  untruncated, first 0 and last 0xffffffff
                np.concatenate([np.arange(size - 1) * 5, [top]]),                # 7  truncated, first 0 and last 0xffffffff
                [],                                                              # 8  lengths 0, 3, 4, 5 and 8 for the quad stream
                [0, 40, 90], [0, 40, 90, 120], [0, 40, 90, 120, 150], [0, 40, 50, 90, 120, 130, 150, 160]]
        qrys = [full[1::3],                                                      # 0  a strict subset of reference 0, untruncated
                [1000, 2000],                                                    # 1  above all of reference 1
                [1, 2, 3, 4, 5, 6],                                              # 2  untruncated
                np.arange(size) * 2,                                             # 3  truncated, first value 0 (= reference 4)
                [0, 2, 5, 2 * size + 10],                                        # 4  untruncated (= reference 3)
                np.concatenate([np.arange(size - 1) * 4 + 1, [5000]]),           # 5  truncated, last 5000 as reference 5
                [0, 5, top],                                                     # 6
                np.concatenate([np.arange(size - 1) * 10, [top]]),               # 7  truncated, first 0 and last 0xffffffff
                [0, 40, 90, 120, 150, 160]]                                      # 8  against the short references
        ref, ref_len = make_signatures(refs, size)
        qry, qry_len = make_signatures(qrys, size)
        assert ref_len.tolist()[:8] == [size, size, 4, 4, size, size, 3, size] and ref_len.tolist()[8:] == [0, 3, 4, 5, 8]
        n_ref, n_qry = len(refs), len(qrys)
        cells = cells_of(ref, ref_len, qry, qry_len)
        hundred = bits(100.0)
        for shape in (None, "square", "thin"):
            set_env(monkeypatch, SHAPE, shape)
            got = {}
            for mode in MODES:
                got[mode] = engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 16, mode)
                same(got[mode], expected(cells, n_ref, n_qry, 16, 16, mode, 1, 0.0)[0])
            assert engine.signature_screen_tile() == ((16, 16) if shape == "square" else (1, 64))
            ident = lambda sh, d: bits(identity_expected(sh, d, 16))
            # a strict subset of a truncated reference: all of the query is in it; the Mash estimate says less
            lq = len(qrys[0])
            assert 0 < lq < size and record(got[QUERY], 0, 0) == (lq, lq, hundred)
            assert record(got[REF], 0, 0) == (lq, size, ident(lq, size)) and record(got[MAX], 0, 0) == (lq, lq, hundred)
            mash = record(engine.signature_screen(ref, ref_len, qry, qry_len, 16, 16), 0, 0)
            assert mash[:2] == (lq, size) and mash[2] < hundred
            # a truncated reference whose last value is below the query's first: nothing shared, no candidate
            assert cells[1][1] == (0, 0, size) and all(record(got[m], 1, 1) is None for m in MODES)
            # both untruncated: the whole lengths
            assert [record(got[m], 2, 2) for m in MODES] == [(3, 6, ident(3, 6)), (3, 4, ident(3, 4)), (3, 4, ident(3, 4))]
            # a truncated query and an untruncated reference: all of the query, the reference up to the query's last value
            assert [record(got[m], 3, 3) for m in MODES] == [(2, size, ident(2, size)), (2, 3, ident(2, 3)), (2, 3, ident(2, 3))]
            # ... and the reverse
            assert [record(got[m], 4, 4) for m in MODES] == [(2, 3, ident(2, 3)), (2, size, ident(2, size)), (2, 3, ident(2, 3))]
            # equal last values, both truncated: everything on both sides
            sh = cells[5][5][0]
            assert 2 <= sh < size and cells[5][5] == (sh, size, size)
            assert [record(got[m], 5, 5) for m in MODES] == [(sh, size, ident(sh, size))] * 3
            # first value 0 and last value 0xffffffff
            assert [record(got[m], 6, 6) for m in MODES] == [(2, 3, ident(2, 3))] * 3
            sh = cells[7][7][0]
            assert sh >= 3 and [record(got[m], 7, 7) for m in MODES] == [(sh, size, ident(sh, size))] * 3
            assert cells[6][7][0] >= 2 and record(got[QUERY], 6, 7) == (cells[6][7][0], 3, ident(cells[6][7][0], 3))
            # reference lengths 0, 3, 4, 5 and 8: a first value of 0 is a value, a zero of the tail is none
            assert all(record(got[m], 8, 8) is None for m in MODES)
            for r, (lr, sh) in zip((9, 10, 11, 12), ((3, 3), (4, 4), (5, 5), (8, 6))):
                assert [record(got[m], 8, r) for m in MODES] == [(sh, 6, ident(sh, 6)), (sh, lr, ident(sh, lr)), (sh, min(6, lr), ident(sh, min(6, lr)))]
            assert record(got[QUERY], 1, 9) is None and record(got[QUERY], 2, 9) is None            # (a zero of the tail is not the value 0)


def test_directed_rows_cpu_build(emu_engine, monkeypatch):
    directed_rows(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_directed_rows_gpu(gpu_engine, monkeypatch):
    directed_rows(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. strips and shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def strips_and_shapes(engine, monkeypatch):
    """every strip height x every prefix of the queries x three reference counts (none a multiple of a tile's references), under the
    shape the strip height selects and under either forced shape: one result per mode"""
    sig, length = small_data()
    more = make_signatures([np.arange(i, i + 9) * 70001 for i in range(25)], 16)
    all_ref, all_len = np.concatenate([sig[:40], more[0]]), np.concatenate([length[:40], more[1]])
    qry, qry_len = sig[40:], length[40:]
    cells = cells_of(all_ref, all_len, qry, qry_len)
    turn, tiles, modes = 0, set(), set()
    for n_ref in (1, 40, 65):
        ref, ref_len = all_ref[:n_ref], all_len[:n_ref]
        for n_qry in (1, 4, 5, 16, 17, 23):
            for strip in STRIPS:
                k, mi, mode = (1, 3, 8, 39, 64)[turn % 5], (0.0, 70.0, 100.0)[turn % 3], MODES[turn % 7 % 3]
                turn += 1
                modes.add((mode, n_ref, n_qry))
                want, _ = expected(cells, n_ref, n_qry, 16, k, mode, 1, mi)
                for shape in (None, "square", "thin"):
                    set_env(monkeypatch, STRIP, strip)
                    set_env(monkeypatch, SHAPE, shape)
                    same(engine.signature_screen_contain(ref, ref_len, qry[:n_qry], qry_len[:n_qry], 16, k, mode, 1, mi), want)
                    assert engine.signature_screen_strips() == strips_of(strip, n_qry), (strip, n_qry)
                    tile = engine.signature_screen_tile()
                    if shape is None:                                  # the last strip's height decides: below the 16 of this pitch, the thin tile
                        h = n_qry if strip is None else min(strip, n_qry)
                        last = n_qry - (n_qry - 1) // h * h
                        assert tile == ((1, 64) if last < 16 else (16, 16)), (tile, strip, n_qry)
                    else:
                        assert tile == ((1, 64) if shape == "thin" else (16, 16))
                    tiles.add((shape, tile))
    assert {t for s, t in tiles if s is None} == {(1, 64), (16, 16)}                 # both shapes ran unforced
    assert {m for m, _, _ in modes} == set(MODES) and len(modes) == 3 * 6 * 3        # every mode at every pair of counts


def test_strips_and_shapes_cpu_build(emu_engine, monkeypatch):
    strips_and_shapes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_strips_and_shapes_gpu(gpu_engine, monkeypatch):
    strips_and_shapes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pitch classes
# ---------------------------------------------------------------------------------------------------------------------------------
def pitch_classes(engine, monkeypatch):
    """9 references x 3 queries at a size of every pitch class (<= 256, <= 1024, <= 2048, above): the thin tile by the strip height, the
    square tile of the class forced; against numpy alone.  1000, 1024, 2048 and 4096 besides: an even number of quads per row, which the
    square tile keeps at a pitch of its own in LDS, and the largest rows of each class."""
    rng = np.random.default_rng(53)
    set_env(monkeypatch, STRIP, None)
    for size, universe, square in ((16, 40, 16), (300, 900, 16), (1100, 4000, 8), (2100, 7000, 4), (1000, 3500, 16), (1024, 3500, 16), (2048, 7000, 8),
                                   (4096, 13000, 4)):
        sets = [rng.choice(universe, size=int(rng.integers(size * 4 // 5, size * 4 // 3)), replace=False) * 300007 for _ in range(12)]
        sets[9] = sets[4]                                                            # query 0 is reference 4
        sets[10] = sets[10][: size // 3]                                             # a short query
        sig, length = make_signatures(sets, size)
        ref, ref_len, qry, qry_len = sig[:9], length[:9], sig[9:], length[9:]
        assert (ref_len == size).any() and (ref_len < size).any() and qry_len[1] < size
        cells = cells_of(ref, ref_len, qry, qry_len)
        assert len({c[0] for row in cells for c in row} - {0}) >= 2
        assert cells[0][4] == (length[4], length[4], length[4])
        turns = ((3, 0.0), (11, 70.0)) if size <= 2100 else ((11, 70.0),)
        for k, mi in turns:
            for mode in MODES:
                want, _ = expected(cells, 9, 3, 16, k, mode, 1, mi)
                for shape, tile in ((None, (1, 64)), ("square", (square, square)), ("thin", (1, 64))):
                    set_env(monkeypatch, SHAPE, shape)
                    same(engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, k, mode, 1, mi), want)
                    assert engine.signature_screen_tile() == tile, (size, shape)


def test_pitch_classes_cpu_build(emu_engine, monkeypatch):
    pitch_classes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_pitch_classes_gpu(gpu_engine, monkeypatch):
    pitch_classes(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. symmetry
# ---------------------------------------------------------------------------------------------------------------------------------
def symmetry(engine, monkeypatch):
    """the sets swapped: QUERY mode of (q, r) is REF mode of (r, q), MAX mode is itself"""
    sig, length = small_data()
    a, a_len, b, b_len = sig[:40], length[:40], sig[40:], length[40:]
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    k = 64                                                                           # >= both set sizes: no cut
    seen = 0
    for one, other in ((QUERY, REF), (REF, QUERY), (MAX, MAX)):
        fwd = engine.signature_screen_contain(a, a_len, b, b_len, 16, k, one)        # queries b against references a
        rev = engine.signature_screen_contain(b, b_len, a, a_len, 16, k, other)      # queries a against references b
        assert fwd[1].sum() == rev[1].sum() > 0
        for q in range(len(b)):
            for r in range(len(a)):
                x = record(fwd, q, r)
                assert x == record(rev, r, q)
                seen += x is not None
        assert seen > 0
    cells = cells_of(a, a_len, b, b_len)
    assert any(c[1] != c[2] for row in cells for c in row if c[0])                   # (the two denominators do differ in this data)


def test_symmetry_cpu_build(emu_engine, monkeypatch):
    symmetry(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_symmetry_gpu(gpu_engine, monkeypatch):
    symmetry(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def arguments(engine):
    ref, ref_len = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    qry, qry_len = make_signatures([[2, 3, 4], [7, 8]], 3)
    lib, h = engine.lib, engine.h
    out, cnt = np.zeros(4, dtype=NEIGHBOR_DT), np.full(2, -7, np.int32)
    out[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)

    def call(n_ref=3, n_qry=2, size=3, kmer=16, ms=1, mi=0.0, k=2, mode=0, ref_p=ref.ctypes.data, rlen_p=ref_len.ctypes.data, qry_p=qry.ctypes.data,
             qlen_p=qry_len.ctypes.data, out_p=out.ctypes.data, cnt_p=cnt.ctypes.data, ctx=h):
        return lib.ani_signature_screen_contain(ctx, ref_p, rlen_p, n_ref, qry_p, qlen_p, n_qry, size, kmer, ms, ctypes.c_float(mi), k, mode, out_p, cnt_p)

    # query [2, 3, 4] (truncated) against [1, 2, 3] (truncated): shared 2; of the query, 2 and 3 are <= 3; of the reference, all are <= 4
    assert call() == 0 and cnt.tolist() == [2, 0]
    assert out.tolist() == [(0, 2, 2, 100.0), (1, 3, 3, 100.0), (-1, 0, 0, 0.0), (-1, 0, 0, 0.0)]
    assert call(mode=1) == 0 and cnt.tolist() == [2, 0]
    assert out.tolist() == [(1, 3, 3, 100.0), (0, 2, 3, float(identity_expected(2, 3, 16))), (-1, 0, 0, 0.0), (-1, 0, 0, 0.0)]
    assert call(mode=2) == 0 and out.tolist()[:2] == [(0, 2, 2, 100.0), (1, 3, 3, 100.0)]
    assert lib.ani_signature_screen_strips(h) == 1
    # rule 7: the mode, and every case of ani_signature_screen's rule 4, one at a time
    for mode in (-1, 3):
        assert call(mode=mode) == -1, mode
        with pytest.raises(AniError) as ex:
            engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, mode)
        assert ex.value.code == -1
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for kmer in (0, -3, 17):
        assert call(kmer=kmer) == -1, kmer
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for mi in (-1.0, 100.5, float("nan")):
        assert call(mi=mi) == -1, mi
    for k in (0, -1, 1025):
        assert call(k=k) == -1, k
    assert call(n_ref=-1) == -1 and call(n_qry=-1) == -1
    for null in ("ref_p", "rlen_p", "qry_p", "qlen_p", "out_p", "cnt_p", "ctx"):
        assert call(**{null: None}) == -1, null
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.signature_screen_contain(ref, np.array(bad_len, dtype=np.int32), qry, qry_len, 16, 2)
        assert ex.value.code == -1, bad_len
    for bad_len in ([4, 2], [3, -1]):
        with pytest.raises(AniError) as ex:
            engine.signature_screen_contain(ref, ref_len, qry, np.array(bad_len, dtype=np.int32), 16, 2)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = ref.copy()
        x[1] = bad_row                                                 # a reference that does not ascend
        with pytest.raises(AniError) as ex:
            engine.signature_screen_contain(x, ref_len, qry, qry_len, 16, 2)
        assert ex.value.code == -1, bad_row
        y = qry.copy()
        y[0] = bad_row                                                 # a query that does not ascend
        with pytest.raises(AniError) as ex:
            engine.signature_screen_contain(ref, ref_len, y, qry_len, 16, 2, "max")
        assert ex.value.code == -1, bad_row
    with pytest.raises(AniError) as ex:                                # ... and with no reference to compare it with
        engine.signature_screen_contain(ref[:0], ref_len[:0], np.array([[3, 2, 1]], np.uint32), np.array([3], np.int32), 16, 2)
    assert ex.value.code == -1
    with pytest.raises(ValueError):                                    # the two sizes must agree
        engine.signature_screen_contain(ref, ref_len, np.zeros((2, 4), np.uint32), qry_len, 16, 2)
    # the limits and the order of the checks: scalars before anything is read or allocated
    assert call(n_ref=(1 << 30) + 1, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == -4
    assert call(n_qry=(1 << 30) + 1, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == -4
    assert call(n_ref=(1 << 30) + 1, mode=3) == -1 and call(n_ref=(1 << 30) + 1, k=0) == -1
    # no queries -> ANI_OK after the scalar checks, nothing read or written, null pointers allowed
    out[:], cnt[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT), -7
    before = (out.copy(), cnt.copy())
    for n_ref in (3, 0):
        assert call(n_ref=n_ref, n_qry=0) == 0
        assert call(n_ref=n_ref, n_qry=0, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == 0
        assert lib.ani_signature_screen_strips(h) == 0
        assert call(n_ref=n_ref, n_qry=0, mode=3) == -1 and call(n_ref=n_ref, n_qry=0, mode=-1) == -1 and call(n_ref=n_ref, n_qry=0, k=0) == -1
    assert np.array_equal(out, before[0]) and np.array_equal(cnt, before[1])
    nb, count = engine.signature_screen_contain(ref, ref_len, qry[:0], qry_len[:0], 16, 3)
    assert nb.shape == (0, 3) and nb.dtype == NEIGHBOR_DT and count.shape == (0,)
    # no references -> every count 0, every slot unused; the reference pointers may be null
    assert call(n_ref=0, ref_p=None, rlen_p=None) == 0
    assert cnt.tolist() == [0, 0] and (out == UNUSED).all()
    nb, count = engine.signature_screen_contain(ref[:0], ref_len[:0], qry, qry_len, 16, 5, "reference")
    assert count.tolist() == [0, 0] and nb.shape == (2, 5) and (nb == UNUSED).all()
    # the mode by name
    for name, mode in (("query", 0), ("reference", 1), ("max", 2)):
        same(engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, name), engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, mode))
    assert engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, "reference")[0][0, 0]["neighbor"] == 1          # (not the default's answer)
    same(engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2), engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, "query"))
    for name in ("Query", "ref", "", "jaccard"):
        with pytest.raises(ValueError):
            engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, 2, name)


def test_arguments_cpu_build(emu_engine):
    arguments(emu_engine)


@pytest.mark.gpu
def test_arguments_gpu(gpu_engine):
    arguments(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def signatures_of(engine, genomes, size):
    sk = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes)
    sig = sk.signatures(size)
    sk.close()
    return sig


def run_cli(binary, engine, tmp, n_len):
    _, paths, genomes = two_genera(tmp, n_len)
    source = 1                                                         # the fragment: a contiguous quarter of genome 1
    piece = genomes[source][0][n_len // 2: n_len // 2 + n_len // 4]
    frag = os.path.join(tmp, "fragment.fa")
    orc.write_fasta(frag, [piece], names=["part"])
    refs, size, k = [0, 1, 3, 4], 200, 3
    qpaths, qgenomes = [frag, paths[2], paths[5]], [[piece], genomes[2], genomes[5]]
    rl, ql = os.path.join(tmp, "r.txt"), os.path.join(tmp, "q.txt")
    open(rl, "w").write("".join(paths[i] + "\n" for i in refs))
    open(ql, "w").write("".join(p + "\n" for p in qpaths))
    common = ["--ql", ql, "--rl", rl, "--sketchScreen", str(k), "--sketchSize", str(size), "--sketchMinANI", "0"]

    (ref, ref_len), (qry, qry_len) = signatures_of(engine, [genomes[i] for i in refs], size), signatures_of(engine, qgenomes, size)
    assert (ref_len == size).all()                                     # the references' signatures are truncated
    firsts = {}
    for mode in ("query", "reference", "max"):
        o = os.path.join(tmp, mode + ".out")
        r = run(binary, common + ["--sketchContain", mode, "-o", o], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 0, (mode, r.stderr.decode()[-2000:])
        assert b"sketch screen done" in r.stderr and b"sketch screen written" in r.stderr
        nb, count = engine.signature_screen_contain(ref, ref_len, qry, qry_len, 16, k, mode, 1, 0.0)
        want = []
        for q, qp in enumerate(qpaths):
            want += ["%s\t%s\t%s\t%d/%d\n" % (qp, paths[refs[x["neighbor"]]], "%g" % x["identity"], x["shared"], x["size"]) for x in nb[q, :count[q]]] \
                or ["%s\tNA\tNA\tNA\n" % qp]
        text = open(o + ".screen").read()
        assert text == "".join(want), mode
        assert count[0] >= 1
        firsts[mode] = text.splitlines()[0].split("\t")
    # the fragment's first line names its source, and the estimate there is above the one the run without the option prints for the pair
    o = os.path.join(tmp, "mash.out")
    assert run(binary, common + ["-o", o]).returncode == 0
    mash = [ln.split("\t") for ln in open(o + ".screen").read().splitlines() if ln.split("\t")[:2] == [frag, paths[source]]]
    assert len(mash) == 1
    assert firsts["query"][:2] == [frag, paths[source]]
    assert float(firsts["query"][2]) >= float(mash[0][2]) and float(firsts["query"][2]) > float(mash[0][2]), (firsts["query"], mash[0])
    shared, d = (int(x) for x in firsts["query"][3].split("/"))
    assert 0 < d < size and int(mash[0][3].split("/")[1]) == size      # the denominator: the part of the fragment's sketch in the reference's range
    # the option alone, and an unknown mode, are refused by name
    bad = os.path.join(tmp, "bad.out")
    r = run(binary, ["--ql", ql, "--rl", rl, "--sketchContain", "query", "-o", bad])
    assert r.returncode != 0 and b"--sketchContain needs --sketchScreen" in r.stderr, r.stderr[-300:]
    r = run(binary, common + ["--sketchContain", "jaccard", "-o", bad])
    assert r.returncode != 0 and b"--sketchContain takes query or reference or max" in r.stderr, r.stderr[-300:]
    assert not os.path.exists(bad) and not os.path.exists(bad + ".screen")
    assert b"--sketchContain" in run(binary, ["-h"]).stdout


def test_cli_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 8000)


@pytest.mark.gpu
def test_cli_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
