"""The device radix sort (kernels/radix.hpp, sort_device.hip) called directly through its extern "C" entry points and compared with
numpy's stable sort: the cases of sort_cases.py, once on the CPU-emulation build (not gpu: a selection, the fiber emulation takes
~0.1 s per call) and once on the product library on an MI355X (gpu: the full cross product of sizes, bit ranges and key
distributions, and one size of 1500 tiles at which the look-back of a tile has to wait for tiles that have not finished)."""
import ctypes
import os

import numpy as np
import pytest

import sort_cases as sc

T = sc.TILE
EMU_RANGES = ((0, 64), (31, 47), (5, 6), (0, 9))        # every size with these,
EMU_SIZES = (sc.WAVE + 1, T + 1, 3 * T + 777)           # every range at these,
EMU_DIST_SIZE = 2 * T + 1                               # every distribution at this one
ENTRIES = ("range", "bits", "pairs")


def ranges_of(entry, ranges):
    """ani_sort_keys_u64_bits / ani_sort_pairs_u64_u32 take the ranges that start at bit 0"""
    return [r for r in ranges if entry == "range" or r[0] == 0]


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    lib = sc.bind(ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libfastani_emu.so")))

    def alloc(nbytes):
        a = np.zeros(nbytes, dtype=np.uint8)
        return a, a.ctypes.data

    def upload(buf, host):
        buf[:] = host

    return lib, (alloc, upload, np.copy)


@pytest.mark.parametrize("n", sc.SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_emu_sizes(emu, entry, n):
    for bit_range in ranges_of(entry, EMU_RANGES):
        for dist in ("uniform", "three") if entry == "range" else ("three",):
            sc.case_array(*emu, entry, n, bit_range, dist)


@pytest.mark.parametrize("entry,bit_range", [(e, r) for e in ENTRIES for r in ranges_of(e, sc.RANGES)], ids=lambda v: v if isinstance(v, str) else "%d-%d" % v)
def test_emu_ranges(emu, entry, bit_range):
    for n in EMU_SIZES:
        for dist in ("uniform", "three") if entry == "range" else ("three",):
            sc.case_array(*emu, entry, n, bit_range, dist)


@pytest.mark.parametrize("dist", sc.DISTS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_emu_distributions(emu, entry, dist):
    for bit_range in ranges_of(entry, EMU_RANGES):
        sc.case_array(*emu, entry, EMU_DIST_SIZE, bit_range, dist)


@pytest.mark.parametrize("n", sc.SIZES)
def test_emu_index(emu, n):
    sc.case_index(*emu, n, "min24")


@pytest.mark.parametrize("n", (2 * T + 1, 3 * T + 777))
def test_emu_index_repeated_hashes(emu, n):
    sc.case_index(*emu, n, "repeats")


def test_emu_async(emu):
    sc.case_async(*emu)


def test_emu_arguments(emu):
    sc.case_arguments_clamped(*emu)
    sc.case_arguments_refused(*emu)
    sc.case_index_arguments(*emu)


def test_emu_determinism(emu):
    sc.case_determinism(*emu, 3 * T + 777)


# ---- the product library on the device ----
SIZE_CLASSES = {"wave": sc.SIZES[0:5], "workgroup": sc.SIZES[5:8], "tile": sc.SIZES[8:11], "tiles": sc.SIZES[11:14]}
# the size that makes tiles wait on each other: the reference sort takes about a second there, so a case is an item
BIG_CASES = (("range", (31, 47), "three"), ("range", (0, 9), "equal"), ("range", (31, 64), "rare"), ("range", (7, 24), "reverse"),
             ("range", (63, 64), "sorted"), ("bits", (0, 9), "three"), ("bits", (0, 64), "rare"), ("pairs", (0, 1), "uniform"),
             ("pairs", (0, 64), "equal"))


@pytest.fixture(scope="module")
def gpu(gpu_engine):
    import torch
    from fastani_amd import _lib
    lib = sc.bind(_lib.load())
    dev = torch.device("cuda", 0)

    def alloc(nbytes):
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return t, t.data_ptr()

    def upload(buf, host):
        buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize(dev)

    def download(buf):
        torch.cuda.synchronize(dev)
        return buf.cpu().numpy()

    return lib, (alloc, upload, download)


@pytest.mark.gpu
@pytest.mark.parametrize("size_class", SIZE_CLASSES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_cross_product(gpu, entry, size_class):
    for n in SIZE_CLASSES[size_class]:
        for bit_range in ranges_of(entry, sc.RANGES):
            for dist in sc.DISTS:
                sc.case_array(*gpu, entry, n, bit_range, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,bit_range,dist", BIG_CASES, ids=lambda v: v if isinstance(v, str) else "%d-%d" % v)
def test_gpu_many_tiles(gpu, entry, bit_range, dist):
    sc.case_array(*gpu, entry, sc.BIG_SIZE, bit_range, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("size_class", SIZE_CLASSES)
def test_gpu_index(gpu, size_class):
    for n in SIZE_CLASSES[size_class]:
        for dist in sc.INDEX_DISTS:
            sc.case_index(*gpu, n, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", sc.INDEX_DISTS)
def test_gpu_index_many_tiles(gpu, dist):
    sc.case_index(*gpu, sc.BIG_SIZE, dist)


@pytest.mark.gpu
def test_gpu_async(gpu):
    sc.case_async(*gpu)
    sc.case_async(*gpu, n=100 * T + 1)


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    sc.case_arguments_clamped(*gpu)
    sc.case_arguments_refused(*gpu)
    sc.case_index_arguments(*gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("uniform", "three"))
def test_gpu_determinism(gpu, which):
    """the largest uniform and the largest three-value case, three times each into fresh outputs"""
    sc.case_determinism(*gpu, sc.BIG_SIZE, which)
