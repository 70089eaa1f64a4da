"""The bootstrap replicate records (kernels/boot.hpp: k_boot_records behind the intervals' k_ci_flags and k_ci_list, launched by
reduce_stage through boot_stage; the ani_sketch_boot_* calls of engine_map.hip) against the numpy restatement of their rules in
boot_cases.py — built from the draws and fix of ci_cases.py and first held to the intervals' restatement on the CPU alone — on the
synthetic lists and the reference layout of reduce_cases.py, through ani_compute_cgi (one query), a sweep over the replicates (every
stride border of a workgroup of 256 and a wave of 64), ani_reduce_check (several queries in one table, with and without the gate), the
gate's edges, the pool path (ANI_TEST_BOOT_LDS_CELLS at 1, 63 and 64), two records per launch (ANI_TEST_BOOT_PIECE), seeds, the
intervals beside them at the same and at another seed (rule 2), the life cycle and the argument checks, with every other mode beside
them, and end to end through ani_map_cgi_batch and ani_map_cgi_fragsets with a default engine, one of many sub-batches, a chunked and a
streamed reference set — once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu).  Every
comparison of the engine is on bits."""
import pytest

import boot_cases as bc
import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_profile import E2E_CONFIGS, ProfileWorld
from test_reducer import CONFIGS, MANY_CONFIGS

ONE_CASES = [(c, name) for c in CONFIGS for name in bc.LISTS_ONE]
ENVS = {
    "lds1": dict(ANI_TEST_BOOT_LDS_CELLS=1), "lds63": dict(ANI_TEST_BOOT_LDS_CELLS=63), "lds64": dict(ANI_TEST_BOOT_LDS_CELLS=64),
    "piece": dict(ANI_TEST_BOOT_PIECE=2),
    "piece_lds": dict(ANI_TEST_BOOT_PIECE=2, ANI_TEST_BOOT_LDS_CELLS=63),   # 128 pool cells a piece: the 129-cell genome is a piece of its own
}


class BootWorld(ProfileWorld):
    """... and engines with a lowered LDS cap and with two records per launch and copy"""

    def engine(self, config):
        if config in ENVS:
            if config not in self.engines:
                with pytest.MonkeyPatch.context() as mp:
                    self.engines[config] = self.make_engine(mp, **ENVS[config])
            return self.engines[config]
        return super().engine(config)

    def end_to_end(self, config):
        if self.e2e is None:
            self.e2e = bc.EndToEnd(self.default_engine)
        return super().end_to_end(config)


# ---- the restatement on its own: CPU only, no engine ----
@pytest.mark.parametrize("name", ("random", "ties", "dense", "low_bits", "all_equal", "n1"))
def test_restatement(name):
    bc.case_restatement(name)


def test_boot_identity():
    bc.case_identity()


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = BootWorld(_emu_engine_with, emu_engine)
    yield w
    w.close()


@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_one_query(emu, config, frag_len, name):
    bc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("replicates", bc.SWEEP_B)
def test_emu_sweep(emu, replicates):
    bc.case_sweep(emu.ref("default", 1000), replicates)


@pytest.mark.parametrize("name", bc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    bc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", bc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate(emu, config, frag_len, name):
    bc.case_many(emu.ref(config, frag_len), name, gated=True)


@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate_edges(emu, config):
    bc.case_gate_edges(emu.ref(config, 1000))


@pytest.mark.parametrize("name", ("dense", "random"))
@pytest.mark.parametrize("config", ("lds1", "lds63", "lds64"))
def test_emu_pool_path(emu, config, name):
    bc.case_many(emu.ref(config, 1000), name, also=emu.ref("default", 1000))


@pytest.mark.parametrize("name", ("random", "dense"))
@pytest.mark.parametrize("config", ("piece", "piece_lds"))
def test_emu_pieces(emu, config, name):
    bc.case_many(emu.ref(config, 1000), name)


def test_emu_seeds(emu):
    bc.case_seeds(emu.ref("default", 1000))


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_intervals(emu, config):
    bc.case_intervals(emu.ref(config, 1000))


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    bc.case_life_cycle(emu.ref(config, 1000))


def test_emu_destroy_while_on(emu):
    bc.case_destroy_while_on(emu.default_engine)


def test_emu_arguments(emu):
    bc.case_arguments(emu.ref("default", 1000))


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_together(emu, config):
    bc.case_together(emu.ref(config, 1000))


@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_emu_end_to_end(emu, config):
    e2e, engine = emu.end_to_end(config)
    e2e.run(engine, config)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = BootWorld(_engine_with, gpu_engine)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_one_query(gpu, config, frag_len, name):
    bc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("replicates", bc.SWEEP_B)
def test_gpu_sweep(gpu, replicates):
    bc.case_sweep(gpu.ref("default", 1000), replicates)


@pytest.mark.gpu
@pytest.mark.parametrize("name", bc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    bc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", bc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate(gpu, config, frag_len, name):
    bc.case_many(gpu.ref(config, frag_len), name, gated=True)


@pytest.mark.gpu
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate_edges(gpu, config):
    bc.case_gate_edges(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("dense", "random"))
@pytest.mark.parametrize("config", ("lds1", "lds63", "lds64"))
def test_gpu_pool_path(gpu, config, name):
    bc.case_many(gpu.ref(config, 1000), name, also=gpu.ref("default", 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("random", "dense"))
@pytest.mark.parametrize("config", ("piece", "piece_lds"))
def test_gpu_pieces(gpu, config, name):
    bc.case_many(gpu.ref(config, 1000), name)


@pytest.mark.gpu
def test_gpu_seeds(gpu):
    bc.case_seeds(gpu.ref("default", 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_intervals(gpu, config):
    bc.case_intervals(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    bc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_destroy_while_on(gpu):
    bc.case_destroy_while_on(gpu.default_engine)


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    bc.case_arguments(gpu.ref("default", 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_together(gpu, config):
    bc.case_together(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_gpu_end_to_end(gpu, config):
    e2e, engine = gpu.end_to_end(config)
    e2e.run(engine, config)
