"""The per-pair fragment identity distributions (kernels/fragdist.hpp: k_fragdist_flags, k_fragdist_list and k_fragdist_records, launched
by reduce_stage; the ani_sketch_fragdist_* calls of engine_map.hip; --fragDist of the command line) against the numpy restatement of
their rules in fragdist_cases.py — which is first held to the oracle's rows on the CPU alone — on the synthetic lists and the reference
layout of reduce_cases.py, through ani_compute_cgi (one query), ani_reduce_check (several queries in one table, with and without the
gate), the gate's edges, the life cycle and the argument checks, with the conservation profile beside it, with two records per launch
(ANI_TEST_FRAGDIST_PIECE), and end to end through ani_map_cgi_batch and ani_map_cgi_fragsets on small related genomes with a default
engine, one of many sub-batches, a chunked and a streamed reference set — once on the CPU-emulation build (not gpu) and once on the
product library on an MI355X (gpu).  Every comparison is on bits."""
import pytest

import fragdist_cases as fc
import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_profile import E2E_CONFIGS, ProfileWorld
from test_reducer import CONFIGS, MANY_CONFIGS

OTHER_CONFIG_LISTS = ("random", "ties", "dense", "c5", "low_bits")
ONE_CASES = [("default", name) for name in fc.LISTS_ONE] + [(c, name) for c in CONFIGS if c != "default" for name in OTHER_CONFIG_LISTS]


class FragDistWorld(ProfileWorld):
    """... and an engine that takes the records two per launch and copy"""

    def engine(self, config):
        if config == "piece":
            if config not in self.engines:
                with pytest.MonkeyPatch.context() as mp:
                    self.engines[config] = self.make_engine(mp, ANI_TEST_FRAGDIST_PIECE=2)
            return self.engines[config]
        return super().engine(config)

    def end_to_end(self, config):
        if self.e2e is None:
            self.e2e = fc.EndToEnd(self.default_engine)
        return super().end_to_end(config)


# ---- the restatement against the oracle: CPU only, no engine ----
@pytest.mark.parametrize("name", fc.LISTS_RESTATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_restatement(frag_len, name):
    fc.case_restatement(frag_len, name)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = FragDistWorld(_emu_engine_with, emu_engine)
    yield w
    w.close()


@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_one_query(emu, config, frag_len, name):
    fc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_slab_edge(emu, frag_len):
    fc.case_slab_edge(emu.ref("default", frag_len))


@pytest.mark.parametrize("name", fc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    fc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", fc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate(emu, config, frag_len, name):
    fc.case_many(emu.ref(config, frag_len), name, gated=True)


@pytest.mark.parametrize("name", ("random", "dense"))
def test_emu_pieces(emu, name):
    fc.case_many(emu.ref("piece", 1000), name)


@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate_edges(emu, config):
    fc.case_gate_edges(emu.ref(config, 1000))


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    fc.case_life_cycle(emu.ref(config, 1000))


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_with_profile(emu, config):
    fc.case_with_profile(emu.ref(config, 1000))


def test_emu_arguments(emu):
    fc.case_arguments(emu.ref("default", 1000))


@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_emu_end_to_end(emu, config):
    e2e, engine = emu.end_to_end(config)
    e2e.run(engine, config)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = FragDistWorld(_engine_with, gpu_engine)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_one_query(gpu, config, frag_len, name):
    fc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_slab_edge(gpu, frag_len):
    fc.case_slab_edge(gpu.ref("default", frag_len))


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    fc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate(gpu, config, frag_len, name):
    fc.case_many(gpu.ref(config, frag_len), name, gated=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("random", "dense"))
def test_gpu_pieces(gpu, name):
    fc.case_many(gpu.ref("piece", 1000), name)


@pytest.mark.gpu
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate_edges(gpu, config):
    fc.case_gate_edges(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    fc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_with_profile(gpu, config):
    fc.case_with_profile(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    fc.case_arguments(gpu.ref("default", 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_gpu_end_to_end(gpu, config):
    e2e, engine = gpu.end_to_end(config)
    e2e.run(engine, config)


# ---- the command line ----
@pytest.mark.parametrize("mode", sorted(fc.pc.CLI_MODES))
def test_emu_cli(emu_engine, tmp_path, mode):
    import os
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir, "all"])
    fc.case_cli(os.path.join(emu_dir, "fastANI_emu"), emu_engine, str(tmp_path), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(fc.pc.CLI_MODES))
def test_gpu_cli(gpu_engine, tmp_path, mode):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fc.case_cli(os.path.join(root, "fastani_amd", "fastANI"), gpu_engine, str(tmp_path), mode)
