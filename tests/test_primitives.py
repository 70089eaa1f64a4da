"""The device primitives of kernels/common.hpp (wave and workgroup scans, lane exchanges, LDS and register sorts, rotl64 / perm_b32 /
alignbyte) and the device-wide prefix sum (device_scan), each run on its own through the test entry points of prim_check.hip and
held to its definition in numpy: the cases of prim_cases.py — the full cross product of sizes and distributions, one workgroup
per pair — once on the CPU-emulation build (not gpu: the cases, the references and the kernels' control flow; the fibers get through
all of it in seconds) and once on the product library on an MI355X (gpu).

Only the GPU half sees the forms the primitives take under __HIP_DEVICE_COMPILE__ — the DPP and v_permlane*_swap lane_xor, the DPP
scan, readlane / readfirstlane, the alignbit / perm / alignbyte builtins, block_barrier's wait — which the CPU stand-in replaces with
shuffles and shifts."""
import pytest

import prim_cases as pc

KEY_BITS = (32, 64)


def _mem_numpy():
    import numpy as np

    def alloc(nbytes):
        a = np.zeros(nbytes, dtype=np.uint8)
        return a, a.ctypes.data

    def upload(buf, host):
        buf[:] = host

    return alloc, upload, np.copy


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    return pc.bind(emu_engine.lib), _mem_numpy()


@pytest.fixture(scope="module")
def emu_ctx(emu_engine):
    return emu_engine.h


@pytest.mark.parametrize("threads", pc.ANY_THREADS)
def test_emu_wave_scans(emu, threads):
    pc.case_wave_scans(*emu, threads)


def test_emu_block_excl_scan(emu):
    pc.case_block_excl_scan(*emu)


def test_emu_block_maxscan(emu):
    pc.case_block_maxscan(*emu)


@pytest.mark.parametrize("where", ("lds", "global"))
def test_emu_block_array_excl_scan(emu, where):
    pc.case_array_scan(*emu, where)


@pytest.mark.parametrize("threads", pc.ANY_THREADS)
@pytest.mark.parametrize("bits", KEY_BITS)
def test_emu_lane_xor(emu, bits, threads):
    pc.case_lane_xor(*emu, bits, threads)


@pytest.mark.parametrize("threads", pc.ANY_THREADS)
def test_emu_lane_value(emu, threads):
    pc.case_lane_value(*emu, threads)


@pytest.mark.parametrize("bits", KEY_BITS)
def test_emu_wave_uniform(emu, bits):
    pc.case_wave_uniform(*emu, bits)


@pytest.mark.parametrize("bits", KEY_BITS)
def test_emu_block_sort(emu, bits):
    pc.case_block_sort(*emu, "block_sort", bits)


@pytest.mark.parametrize("bits", KEY_BITS)
def test_emu_block_bitonic_sort(emu, bits):
    pc.case_block_sort(*emu, "bitonic", bits)


@pytest.mark.parametrize("kpt", (1, 2, 4))
def test_emu_wave_sort_regs(emu, kpt):
    pc.case_wave_sort(*emu, kpt)


def test_emu_rotl64(emu):
    pc.case_rotl64(*emu)


def test_emu_perm_b32(emu):
    pc.case_perm_b32(*emu)


def test_emu_alignbyte(emu):
    pc.case_alignbyte(*emu)


def test_emu_check_arguments(emu):
    pc.case_arguments(*emu)


@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES)
def test_emu_device_scan(emu, emu_ctx, n):
    pc.case_device_scan(*emu, emu_ctx, n)


def test_emu_device_scan_empty(emu, emu_ctx):
    pc.case_device_scan_empty(*emu, emu_ctx)


@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES[4:])
def test_emu_device_scan_large_totals(emu, emu_ctx, n):
    pc.case_device_scan_large_totals(*emu, emu_ctx, n)


@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES[4:])
def test_emu_device_scan_default_limit(emu, emu_ctx, n):
    pc.case_device_scan_default_limit(*emu, emu_ctx, n)


@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES)
def test_emu_device_scan_caller_limit(emu, emu_ctx, n):
    pc.case_device_scan_caller_limit(*emu, emu_ctx, n)


def test_emu_determinism_sort(emu):
    pc.case_determinism_sort(*emu)


def test_emu_determinism_scan(emu, emu_ctx):
    pc.case_determinism_scan(*emu, emu_ctx)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    import torch
    from fastani_amd import _lib
    lib = pc.bind(_lib.load())
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


@pytest.fixture(scope="module")
def gpu_ctx(gpu_engine):
    return gpu_engine.h


@pytest.mark.gpu
@pytest.mark.parametrize("threads", pc.ANY_THREADS)
def test_gpu_wave_scans(gpu, threads):
    pc.case_wave_scans(*gpu, threads)


@pytest.mark.gpu
def test_gpu_block_excl_scan(gpu):
    pc.case_block_excl_scan(*gpu)


@pytest.mark.gpu
def test_gpu_block_maxscan(gpu):
    pc.case_block_maxscan(*gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("lds", "global"))
def test_gpu_block_array_excl_scan(gpu, where):
    pc.case_array_scan(*gpu, where)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", pc.ANY_THREADS)
@pytest.mark.parametrize("bits", KEY_BITS)
def test_gpu_lane_xor(gpu, bits, threads):
    pc.case_lane_xor(*gpu, bits, threads)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", pc.ANY_THREADS)
def test_gpu_lane_value(gpu, threads):
    pc.case_lane_value(*gpu, threads)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", KEY_BITS)
def test_gpu_wave_uniform(gpu, bits):
    pc.case_wave_uniform(*gpu, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", KEY_BITS)
def test_gpu_block_sort(gpu, bits):
    pc.case_block_sort(*gpu, "block_sort", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", KEY_BITS)
def test_gpu_block_bitonic_sort(gpu, bits):
    pc.case_block_sort(*gpu, "bitonic", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("kpt", (1, 2, 4))
def test_gpu_wave_sort_regs(gpu, kpt):
    pc.case_wave_sort(*gpu, kpt)


@pytest.mark.gpu
def test_gpu_rotl64(gpu):
    pc.case_rotl64(*gpu)


@pytest.mark.gpu
def test_gpu_perm_b32(gpu):
    pc.case_perm_b32(*gpu)


@pytest.mark.gpu
def test_gpu_alignbyte(gpu):
    pc.case_alignbyte(*gpu)


@pytest.mark.gpu
def test_gpu_check_arguments(gpu):
    pc.case_arguments(*gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES)
def test_gpu_device_scan(gpu, gpu_ctx, n):
    pc.case_device_scan(*gpu, gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_device_scan_empty(gpu, gpu_ctx):
    pc.case_device_scan_empty(*gpu, gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES[4:])
def test_gpu_device_scan_large_totals(gpu, gpu_ctx, n):
    pc.case_device_scan_large_totals(*gpu, gpu_ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES[4:])
def test_gpu_device_scan_default_limit(gpu, gpu_ctx, n):
    pc.case_device_scan_default_limit(*gpu, gpu_ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.DEVICE_SCAN_SIZES)
def test_gpu_device_scan_caller_limit(gpu, gpu_ctx, n):
    pc.case_device_scan_caller_limit(*gpu, gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_determinism_sort(gpu):
    """the largest sort case three times into fresh outputs"""
    pc.case_determinism_sort(*gpu)


@pytest.mark.gpu
def test_gpu_determinism_scan(gpu, gpu_ctx):
    """the largest scan case three times into fresh outputs"""
    pc.case_determinism_scan(*gpu, gpu_ctx)
