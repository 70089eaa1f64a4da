"""The per-bin conservation profile (kernels/profile.hpp: k_profile_bins and k_profile_queries, launched by reduce_stage; the
ani_sketch_profile_* calls of engine_map.hip) against the numpy restatement of its rules in profile_cases.py — which is first held to
the oracle's rows on the CPU alone — on the synthetic lists and the reference layout of reduce_cases.py (453 bins: two workgroups of
k_profile_bins, the second partial, genome borders inside a workgroup), through ani_compute_cgi (one query), ani_reduce_check (several
queries in one table, with and without the gate), the life cycle and the argument checks, and end to end through ani_map_cgi_batch and
ani_map_cgi_fragsets on small related genomes with a default engine, one of many sub-batches, a chunked and a streamed reference set —
once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu).  Every comparison is on bits."""
import pytest

import profile_cases as pc
import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_reducer import CONFIGS, MANY_CONFIGS, World

E2E_CONFIGS = ("default", "subbatch", "chunked", "streamed")


class ProfileWorld(World):
    """... and the end-to-end inputs and engines"""

    def __init__(self, make_engine, default_engine):
        super().__init__(make_engine, default_engine)
        self.e2e = None
        self.e2e_engines = {}

    def end_to_end(self, config):
        if self.e2e is None:
            self.e2e = pc.EndToEnd(self.default_engine)
        if config == "default":
            return self.e2e, self.default_engine
        if config not in self.e2e_engines:
            env = dict(ANI_SUBBATCH_FRAGS=50)            # under the 60 fragments of a query genome: a sub-batch per genome, six in all
            if config in ("chunked", "streamed"):
                env = dict(ANI_MAX_INDEX_MINIMIZERS=self.e2e.n_minimizers // 4)
            if config == "streamed":
                env["ANI_MAX_RESIDENT_CHUNKS"] = 1
            with pytest.MonkeyPatch.context() as mp:
                self.e2e_engines[config] = self.make_engine(mp, **env)
        return self.e2e, self.e2e_engines[config]

    def close(self):
        super().close()
        for e in self.e2e_engines.values():
            e.close()


# ---- the restatement against the oracle: CPU only, no engine ----
@pytest.mark.parametrize("name", pc.LISTS_RESTATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_restatement(frag_len, name):
    pc.case_restatement(frag_len, name)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = ProfileWorld(_emu_engine_with, emu_engine)
    yield w
    w.close()


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_layout(emu, config, frag_len):
    pc.case_layout(emu.ref(config, frag_len))


@pytest.mark.parametrize("name", pc.LISTS_ONE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_one_query(emu, config, frag_len, name):
    pc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", pc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    pc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", pc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate(emu, config, frag_len, name):
    pc.case_many(emu.ref(config, frag_len), name, gated=True)


@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate_edges(emu, config):
    pc.case_gate_edges(emu.ref(config, 1000))


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    pc.case_life_cycle(emu.ref(config, 1000))


def test_emu_arguments(emu):
    pc.case_arguments(emu.ref("default", 1000))


@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_emu_end_to_end(emu, config):
    e2e, engine = emu.end_to_end(config)
    e2e.run(engine, config)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = ProfileWorld(_engine_with, gpu_engine)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_layout(gpu, config, frag_len):
    pc.case_layout(gpu.ref(config, frag_len))


@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.LISTS_ONE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_one_query(gpu, config, frag_len, name):
    pc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    pc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate(gpu, config, frag_len, name):
    pc.case_many(gpu.ref(config, frag_len), name, gated=True)


@pytest.mark.gpu
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate_edges(gpu, config):
    pc.case_gate_edges(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    pc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    pc.case_arguments(gpu.ref("default", 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_gpu_end_to_end(gpu, config):
    e2e, engine = gpu.end_to_end(config)
    e2e.run(engine, config)


# ---- the command line ----
@pytest.mark.parametrize("mode", sorted(pc.CLI_MODES))
def test_emu_cli(emu_engine, tmp_path, mode):
    import os
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir, "all"])
    pc.case_cli(os.path.join(emu_dir, "fastANI_emu"), emu_engine, str(tmp_path), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(pc.CLI_MODES))
def test_gpu_cli(gpu_engine, tmp_path, mode):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pc.case_cli(os.path.join(root, "fastani_amd", "fastANI"), gpu_engine, str(tmp_path), mode)
