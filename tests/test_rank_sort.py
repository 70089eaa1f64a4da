"""ani_sort_index_pos (sort_device.hip, kernels/radix.hpp: k_radix_pass<uint32_t, uint32_t, ...>), the index sort whose payload is the
entry's position rank, called directly and compared with numpy's stable argsort of the hashes — once on the CPU-emulation build (not
gpu) and once on the product library on an MI355X (gpu).

Expected: sPos[r] is the rank (the index into mHash / mSeq / mWpos) of the r-th entry in hash order, equal hashes in position order;
sHash the hashes in that order; mHash / mSeq / mWpos what ani_sort_index writes.  Like sort_cases.py every case also checks what the
call writes besides its result: the elements behind every output's n-th, the pieces, the bytes around the workspace.  Every comparison
is exact: a stable sort has one right answer."""
import ctypes

import numpy as np
import pytest

import sort_cases as sc
from test_radix_sort import emu, gpu      # noqa: F401  (the two halves' library and memory)

T = sc.TILE
SIZES = (0, 1, T - 1, T, T + 1, 2 * T + 1, 50021)
PIECES = {1: lambda n: [n], 3: lambda n: [n // 3, 0, n - n // 3], 7: lambda n: [n // 7, T, 5, 0, n // 7 + 1, 1, n - 2 * (n // 7) - T - 7]}


def bind(lib):
    vp, sz, i, psz = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)
    lib.ani_sort_index_pos.argtypes = [ctypes.POINTER(vp), psz, i, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp, vp, psz, vp, vp, vp]
    lib.ani_sort_index_pos.restype = i
    return lib


def index_pos_sort(lib, mem, rec, sizes, seq_base):
    """ani_sort_index_pos over the records `rec` handed over as pieces of `sizes` records"""
    bind(lib)
    n = len(rec)
    what = "index_pos n=%d pieces=%r" % (n, sizes)
    assert sum(sizes) == n and min(sizes) >= 0
    pieces, o = [], 0
    for s in sizes:
        pieces.append(sc.Buf(mem, rec[o:o + s].copy()))
        o += s
    k = len(sizes)
    piece_ptr = (ctypes.c_void_p * k)(*[p.ptr for p in pieces])
    piece_n = (ctypes.c_size_t * k)(*sizes)
    outs = [sc.out_buf(mem, n, t, 51 + j) for j, t in enumerate((np.uint32, np.int32, np.int32, np.uint32, np.uint32, np.uint32, np.uint32))]
    m_hash, m_seq, m_wpos, tmp_k, tmp_v, s_hash, s_pos = outs

    def call(tmp, tmp_bytes):
        return lib.ani_sort_index_pos(piece_ptr, piece_n, k, seq_base, n, m_hash.ptr, m_seq.ptr, m_wpos.ptr, tmp_k.ptr, tmp_v.ptr, s_hash.ptr, s_pos.ptr,
                                      tmp, ctypes.byref(tmp_bytes), None, None, None)

    tmp_bytes = ctypes.c_size_t(0)
    assert call(None, tmp_bytes) == 0, what
    assert tmp_bytes.value > 0, what
    assert all(b.unchanged() for b in outs), "%s: the size query wrote to an output" % what
    ws = sc.Workspace(mem, tmp_bytes.value)
    rc = call(ws.ptr, tmp_bytes)
    assert rc == 0, "%s: returned %d" % (what, rc)
    order = np.argsort(rec[:, 0], kind="stable")
    sc.check_out(m_hash, n, rec[:, 0], what + " mHash")
    sc.check_out(m_seq, n, (rec[:, 1] - np.uint32(seq_base)).astype(np.int32), what + " mSeq")
    sc.check_out(m_wpos, n, rec[:, 2].astype(np.int32), what + " mWpos")
    sc.check_out(s_hash, n, rec[order, 0], what + " sHash")
    sc.check_out(s_pos, n, order.astype(np.uint32), what + " sPos")
    for b, name in ((tmp_k, "tmpK"), (tmp_v, "tmpV")):          # scratch: any content, but only n 32-bit elements of it
        assert np.array_equal(b.get()[n:], b.init[n:]), "%s: written behind the %d-th element of %s" % (what, n, name)
    ws.check_fences(what)
    assert all(p.unchanged() for p in pieces), "%s: a piece was written" % what


def case_sizes(lib, mem, n):
    """one tile +- 1, two tiles + 1, ~50 000 minimizer-like hashes (nine tiles); 0 and 1"""
    index_pos_sort(lib, mem, sc.make_records("min24", n, 1000), sc.split_pieces(n), 1000)


def case_equal(lib, mem):
    """one hash for three tiles: the payload must come out as 0 .. n - 1 (stability inside a tile and across the look-back)"""
    n = 3 * T
    rec = sc.make_records("min24", n, 7)
    rec[:, 0] = 0x00c0ffee
    index_pos_sort(lib, mem, rec, [n], 7)
    rec[:, 0] = np.where(np.arange(n) % 5 == 0, 0xffffffff, 0)   # two hashes at the ends of the range, interleaved
    index_pos_sort(lib, mem, rec, [T + 1, 0, 2 * T - 1], 7)


def case_pieces(lib, mem, k):
    """the same records as 1, 3 and 7 pieces, an empty piece in the middle"""
    n = 2 * T + 1
    for dist in sc.INDEX_DISTS:
        sizes = PIECES[k](n)
        assert sum(sizes) == n and (k == 1 or 0 in sizes[1:-1])
        index_pos_sort(lib, mem, sc.make_records(dist, n, 3), sizes, 3)


def case_retry(lib, mem, monkeypatch):
    """ANI_TEST_SORT_FAIL_EVERY=2: every second completed sort of the process reports a given-up look-back and is repeated once"""
    monkeypatch.setenv("ANI_TEST_SORT_FAIL_EVERY", "2")
    for _ in range(3):                                          # odd or even, the process-wide count meets a failing attempt
        index_pos_sort(lib, mem, sc.make_records("repeats", T + 1, 0), [T + 1], 0)


# ---- the CPU-emulation build ----
@pytest.mark.parametrize("n", SIZES)
def test_emu_sizes(emu, n):
    case_sizes(*emu, n)


def test_emu_equal_hashes(emu):
    case_equal(*emu)


@pytest.mark.parametrize("k", sorted(PIECES))
def test_emu_pieces(emu, k):
    case_pieces(*emu, k)


def test_emu_retry(emu, monkeypatch):
    case_retry(*emu, monkeypatch)


# ---- the product library on the device ----
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_sizes(gpu, n):
    case_sizes(*gpu, n)


@pytest.mark.gpu
def test_gpu_equal_hashes(gpu):
    case_equal(*gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(PIECES))
def test_gpu_pieces(gpu, k):
    case_pieces(*gpu, k)


@pytest.mark.gpu
def test_gpu_retry(gpu, monkeypatch):
    case_retry(*gpu, monkeypatch)
