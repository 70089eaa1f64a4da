"""The hash-ordered payload of an index chunk is the entry's position rank (IndexChunk::sPos, carried through ani_sort_index_pos), and
k_index_links (kernels/index.hpp) takes the two entries of a same-hash pair from it: on the record sets of index_cases.py and on pairs
placed where the rank reject decides — once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu).

ani_index_check: array 11 is sPos itself, array 2 still the 64-bit seqId << 32 | wpos in hash order (expanded for the call).  The
definitions are index_cases.define's; every comparison is exact."""
import ctypes

import numpy as np
import pytest

import index_cases as ic
from test_index_build import emu, gpu      # noqa: F401  (the two halves' World: engines and memory)

S_POS = 11                                                                     # host/engine.hpp: ani_index_check
SETS = ((1, "min_w"), (9, "identical"), (1025, "edge_runs"), (2049, "low"), (20011, "min_w"), (6145, "identical"))


def fetch_pos(ix, chunk):
    size = ctypes.c_uint64(0)
    ix.engine._chk(ix.lib.ani_index_check(ix.engine.h, ix.sk.h, chunk, S_POS, None, 0, ctypes.byref(size)))
    out = np.zeros(size.value // 4, dtype=np.uint32)
    ix.engine._chk(ix.lib.ani_index_check(ix.engine.h, ix.sk.h, chunk, S_POS, out.ctypes.data if out.size else None, out.nbytes, ctypes.byref(size)))
    assert size.value == out.nbytes
    return out


def check_ranks(ix, what):
    """sPos = the stable argsort of the chunk's hashes, and array 2 = (mSeq << 32 | mWpos)[sPos], for every chunk"""
    for chunk, (g0, g1) in enumerate(ix.genome_ranges()):
        rec, _ = ix.rset.chunk(g0, g1)
        order = np.argsort(rec[:, 0], kind="stable")
        pos = fetch_pos(ix, chunk)
        ic.same("%s chunk %d sPos" % (what, chunk), pos, order.astype(np.uint32))
        sw = (rec[:, 1].astype(np.uint64) << np.uint64(32)) | rec[:, 2].astype(np.uint64)
        ic.same("%s chunk %d array 2" % (what, chunk), ix.fetch(chunk, ic.S_SW), sw[pos] if len(pos) else sw)


def case_sets(world, n, dist):
    p, w, cmw = ic.geometry(world.default, 16, 3000)
    ix, _ = ic.check_index(world.default, world.mem, p, ic.general_set(n, dist, 16, w, cmw), what="ranks %s" % dist)
    try:
        check_ranks(ix, "general %s n=%d" % (dist, n))
    finally:
        ix.close()


def case_chunked(world):
    """three or more chunks: the ranks are chunk-local"""
    engine = world.engine(ANI_MAX_INDEX_MINIMIZERS=ic.CHUNKED_MAX_INDEX_MINIMIZERS)
    p, w, cmw = ic.geometry(engine, 16, 3000)
    r = ic.rng(81)
    contigs = [ic.contig(r, ic.draw_hashes(r, ic.CHUNK_GENOME_RECORDS, "min_w", w), cmw, w) for _ in range(6)]
    ix, defs = ic.check_index(engine, world.mem, p, ic.RecordSet(contigs, [1] * 6), chunks=3, what="ranks chunked")
    try:
        assert all(ix.info(c)["c0"] > 0 for c in range(1, len(defs)))
        check_ranks(ix, "chunked")
    finally:
        ix.close()


def case_rank_reject(world, k, frag_len):
    """A dense contig (every position a minimizer, so rank distance = wpos distance): same-hash pairs at rank distance cmw, cmw + 1 (the
    last that is near: wpos[ib] - wpos[ia + 1] = cmw) and cmw + 2 (rejected on the ranks alone).  Then the same distances in a contig
    with one gap inside the pair, where the ranks pass and the positions decide; and the same hash on the last entry of one contig and
    the first of the next (rank distance 1), which is no link."""
    p, w, cmw = ic.geometry(world.default, k, frag_len)
    assert cmw >= 3
    r = ic.rng(82, k, frag_len)
    fresh = iter(ic.draw_hashes(r, 12 * (cmw + 8) + 100, "distinct", w))
    fill = lambda m: np.array([next(fresh) for _ in range(m)], dtype=np.uint32)
    contigs, expect = [], []
    for d in (cmw, cmw + 1, cmw + 2):
        m = d + 11
        h = fill(m)
        h[5 + d] = h[5]
        contigs.append((m + 3, h, np.arange(m) + 2))                           # dense: wpos = rank + 2
        expect.append(d <= cmw + 1)
    for d in (cmw, cmw + 1):                                                   # ranks d apart, one position skipped behind ia + 1: wpos distance d + 1
        m = d + 11
        h = fill(m)
        h[5 + d] = h[5]
        wpos = np.arange(m) + 2
        wpos[7:] += 1
        contigs.append((m + 4, h, wpos))
        expect.append(d + 1 <= cmw + 1)
    ha, hb = fill(9), fill(9)
    hb[0] = ha[-1]                                                             # across the border, rank distance 1
    contigs += [(40, ha, np.arange(9) * 4), (40, hb, np.arange(9) * 4)]
    ix, (d,) = ic.check_index(world.default, world.mem, p, ic.RecordSet(contigs), what="rank reject k=%d L=%d" % (k, frag_len))
    try:
        check_ranks(ix, "rank reject")
        first = d["contigFirstMin"]
        linked = [bool(d["linked"][first[c] + 5]) for c in range(5)]
        assert linked == expect == [True, True, False, True, False], (linked, expect)
        assert d["pairs"] == 5 and d["nearPairs"] == 3                        # (define counts the pairs of one contig)
        border = int(first[6])
        assert not d["linked"][border - 1] and not d["linked"][border]
    finally:
        ix.close()


# ---- the CPU-emulation build ----
@pytest.mark.parametrize("n,dist", SETS)
def test_emu_sets(emu, n, dist):
    case_sets(emu, n, dist)


def test_emu_chunked(emu):
    case_chunked(emu)


@pytest.mark.parametrize("k,frag_len", ((16, 3000), (12, 1000)))
def test_emu_rank_reject(emu, k, frag_len):
    case_rank_reject(emu, k, frag_len)


# ---- the product library on the device ----
@pytest.mark.gpu
@pytest.mark.parametrize("n,dist", SETS)
def test_gpu_sets(gpu, n, dist):
    case_sets(gpu, n, dist)


@pytest.mark.gpu
def test_gpu_chunked(gpu):
    case_chunked(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("k,frag_len", ((16, 3000), (12, 1000)))
def test_gpu_rank_reject(gpu, k, frag_len):
    case_rank_reject(gpu, k, frag_len)
