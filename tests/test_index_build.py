"""The index build after the sort (build_chunk_index, engine_index.hip, with the kernels of kernels/index.hpp: k_index_contig_first,
k_index_links and its rerun, k_table_block_totals / the host carry loop / k_table_scatter, table_probe, k_index_window_links,
k_index_mark_dups, k_index_pos_sample, k_index_mark_shared) on synthetic minimizer records, every array of every index chunk held to
a numpy definition: the cases of index_cases.py — once on the CPU-emulation build (not gpu) and once on the product library on an
MI355X (gpu).  The arrays come out through the test entry points ani_index_check, ani_index_probe_check and ani_index_links_check.

Only the GPU half sees the device form of k_index_window_links (the LDS staging, the non-temporal loads beyond the staged range, the
16-byte loads and stores), the wave shuffles of k_index_links and the atomics of index_link_pair as the hardware runs them.

The chunk's arrays are pool allocations, 16-byte aligned: the kernels' scalar load and store paths are reached at the tails only, not
through misaligned buffers (index_cases.py says where the misaligned form is run).  Every comparison is exact."""
import pytest

import index_cases as ic
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_primitives import _mem_numpy


class World:
    """the default engine and memory of one half, and the engines with their own settings, made when a test first asks for them"""

    def __init__(self, make_engine, default_engine, mem):
        self.make_engine, self.default, self.mem = make_engine, default_engine, mem
        self.engines = {}

    def engine(self, **env):
        key = tuple(sorted(env.items()))
        if key not in self.engines:
            with pytest.MonkeyPatch.context() as mp:      # the engine reads its environment when it is made
                self.engines[key] = self.make_engine(mp, **env)
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()


def run_pair_cap(w):
    ic.case_pair_cap(w.default, w.engine(ANI_TEST_DUP_PAIR_CAP=3), w.mem)


def run_chunked(w):
    ic.case_chunked(w.engine(ANI_MAX_INDEX_MINIMIZERS=ic.CHUNKED_MAX_INDEX_MINIMIZERS), w.mem)


def run_not_resident(w):
    ic.case_not_resident(w.engine(ANI_MAX_INDEX_MINIMIZERS=ic.CHUNKED_MAX_INDEX_MINIMIZERS, ANI_MAX_RESIDENT_CHUNKS=1), w.mem)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = World(_emu_engine_with, emu_engine, _mem_numpy())
    yield w
    w.close()


@pytest.mark.parametrize("dist", ic.DISTS)
@pytest.mark.parametrize("n", ic.SIZES)
def test_emu_general(emu, n, dist):
    ic.case_general(emu.default, emu.mem, n, dist)


@pytest.mark.parametrize("values", ic.RUN_VALUES)
def test_emu_runs(emu, values):
    ic.case_runs(emu.default, emu.mem, values)


@pytest.mark.parametrize("k,frag_len", ic.COMBOS)
def test_emu_near_borders(emu, k, frag_len):
    ic.case_near_borders(emu.default, emu.mem, k, frag_len)


def test_emu_contigs(emu):
    ic.case_contigs(emu.default, emu.mem)


@pytest.mark.parametrize("k,frag_len", ic.COMBOS)
def test_emu_window_links(emu, k, frag_len):
    ic.case_window_links(emu.default, emu.mem, k, frag_len)


def test_emu_pair_cap(emu):
    run_pair_cap(emu)


def test_emu_chunked(emu):
    run_chunked(emu)


def test_emu_not_resident(emu):
    run_not_resident(emu)


def test_emu_arguments(emu):
    ic.case_arguments(emu.default, emu.mem)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    import torch
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

    w = World(_engine_with, gpu_engine, (alloc, upload, download))
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dist", ic.DISTS)
@pytest.mark.parametrize("n", ic.SIZES)
def test_gpu_general(gpu, n, dist):
    ic.case_general(gpu.default, gpu.mem, n, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("values", ic.RUN_VALUES)
def test_gpu_runs(gpu, values):
    ic.case_runs(gpu.default, gpu.mem, values)


@pytest.mark.gpu
@pytest.mark.parametrize("k,frag_len", ic.COMBOS)
def test_gpu_near_borders(gpu, k, frag_len):
    ic.case_near_borders(gpu.default, gpu.mem, k, frag_len)


@pytest.mark.gpu
def test_gpu_contigs(gpu):
    ic.case_contigs(gpu.default, gpu.mem)


@pytest.mark.gpu
@pytest.mark.parametrize("k,frag_len", ic.COMBOS)
def test_gpu_window_links(gpu, k, frag_len):
    ic.case_window_links(gpu.default, gpu.mem, k, frag_len)


@pytest.mark.gpu
def test_gpu_pair_cap(gpu):
    run_pair_cap(gpu)


@pytest.mark.gpu
def test_gpu_chunked(gpu):
    run_chunked(gpu)


@pytest.mark.gpu
def test_gpu_not_resident(gpu):
    run_not_resident(gpu)


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    ic.case_arguments(gpu.default, gpu.mem)
