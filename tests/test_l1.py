"""The L1 stage — seed lookup and candidate regions, kernels/l1.hpp behind l1_stage (the first half of map_stage, engine_map.hip) — on
synthetic index records and hand-written fragment sketches, every output of one call held to the sequential definition of
computeMap.hpp:283-354 (l1_cases.py): the ordered candidates exactly as the L2 half would receive them, fragHits, the probe's
(first, count) per sketch hash and the routing of the fragments to the wave kernel, class S, class M and the batched path — once on the
CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu), through the test entry point ani_l1_check.

The run-rule family (spans of L - 1 and L, the previous end at start - 1 / start / start + 1, the clamp at 0, contig borders,
H = m - 1 / m / m + 1, merge chains) runs once per implementation: the wave kernel at its three sort widths, class S dense and listed,
class M, the noise filter always and never, the batched global-memory path.  Every comparison is exact."""
import pytest

import l1_cases as lc
from test_index_build import emu, gpu      # noqa: F401  (the two halves' World: engines and memory)

PATHS = tuple(lc.PATHS)
OTHER = (("tiny1", 16, 1000), ("classS_dense", 12, 3000), ("big_all", 12, 1000), ("classM", 16, 1000))      # COMBOS of index_cases.py
NFRAG = ((1, 1), (3, 1), (3, 0), (4, 1), (4, 0), (5, 1), (5, 0), (255, 0), (256, 1), (257, 0), (257, 1))
FILTER = (None, 0, 100000)
GENOMES = ((5, 9), (7, 2, 12))


# ---- the CPU-emulation build ----
@pytest.mark.parametrize("path", PATHS)
def test_emu_run_rule(emu, path):
    lc.case_run_rule(emu, path)


@pytest.mark.parametrize("path", ("tiny1", "classS_dense", "big_all"))
def test_emu_run_rule_id95(emu, path):
    lc.case_run_rule(emu, path, identity=95.0, sizes=lc.FAMILY_95)


@pytest.mark.parametrize("path,k,frag_len", OTHER)
def test_emu_run_rule_geometry(emu, path, k, frag_len):
    lc.case_run_rule(emu, path, k=k, L=frag_len, sizes=lc.FAMILY_GEOMETRY)


@pytest.mark.parametrize("tiny", (1, 0))
def test_emu_class_borders(emu, tiny):
    lc.case_class_borders(emu, tiny)


@pytest.mark.parametrize("frag_len", (3000, 1000))
@pytest.mark.parametrize("filter_min", FILTER)
def test_emu_noise_filter(emu, filter_min, frag_len):
    lc.case_noise_filter(emu, filter_min, L=frag_len)


def test_emu_big_key_widths(emu):
    lc.case_big_key_widths(emu)


def test_emu_big_tiles(emu):
    lc.case_big_tiles(emu)


def test_emu_big_groups(emu):
    lc.case_big_groups(emu)


@pytest.mark.parametrize("n_frag,mostly_small", NFRAG)
def test_emu_launch_shape(emu, n_frag, mostly_small):
    lc.case_launch_shape(emu, n_frag, mostly_small)


@pytest.mark.parametrize("genome_fragments", GENOMES)
def test_emu_genomes(emu, genome_fragments):
    lc.case_genomes(emu, genome_fragments)


def test_emu_pool_retry(emu):
    lc.case_pool_retry(emu)


def test_emu_hit_limit(emu):
    lc.case_hit_limit(emu)


def test_emu_max_s(emu):
    lc.case_max_s(emu)


def test_emu_chunks(emu):
    lc.case_chunks(emu)


def test_emu_arguments(emu):
    lc.case_arguments(emu)


# ---- the product library on the device ----
@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_gpu_run_rule(gpu, path):
    lc.case_run_rule(gpu, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ("tiny1", "classS_dense", "big_all"))
def test_gpu_run_rule_id95(gpu, path):
    lc.case_run_rule(gpu, path, identity=95.0, sizes=lc.FAMILY_95)


@pytest.mark.gpu
@pytest.mark.parametrize("path,k,frag_len", OTHER)
def test_gpu_run_rule_geometry(gpu, path, k, frag_len):
    lc.case_run_rule(gpu, path, k=k, L=frag_len, sizes=lc.FAMILY_GEOMETRY)


@pytest.mark.gpu
@pytest.mark.parametrize("tiny", (1, 0))
def test_gpu_class_borders(gpu, tiny):
    lc.case_class_borders(gpu, tiny)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", (3000, 1000))
@pytest.mark.parametrize("filter_min", FILTER)
def test_gpu_noise_filter(gpu, filter_min, frag_len):
    lc.case_noise_filter(gpu, filter_min, L=frag_len)


@pytest.mark.gpu
def test_gpu_big_key_widths(gpu):
    lc.case_big_key_widths(gpu)


@pytest.mark.gpu
def test_gpu_big_tiles(gpu):
    lc.case_big_tiles(gpu)


@pytest.mark.gpu
def test_gpu_big_groups(gpu):
    lc.case_big_groups(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n_frag,mostly_small", NFRAG)
def test_gpu_launch_shape(gpu, n_frag, mostly_small):
    lc.case_launch_shape(gpu, n_frag, mostly_small)


@pytest.mark.gpu
@pytest.mark.parametrize("genome_fragments", GENOMES)
def test_gpu_genomes(gpu, genome_fragments):
    lc.case_genomes(gpu, genome_fragments)


@pytest.mark.gpu
def test_gpu_pool_retry(gpu):
    lc.case_pool_retry(gpu)


@pytest.mark.gpu
def test_gpu_hit_limit(gpu):
    lc.case_hit_limit(gpu)


@pytest.mark.gpu
def test_gpu_max_s(gpu):
    lc.case_max_s(gpu)


@pytest.mark.gpu
def test_gpu_chunks(gpu):
    lc.case_chunks(gpu)


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    lc.case_arguments(gpu)
