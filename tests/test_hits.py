"""The reciprocal best-hit records (kernels/hits.hpp: k_hits_owner, k_hits_claim, k_hits_flags, k_hits_list and k_hits_records, launched by
reduce_stage; the ani_sketch_hits_* calls of engine_map.hip; --hits of the command line) against the numpy restatement of their rules
in hits_cases.py — which is first held to the oracle's rows on the CPU alone — on the synthetic lists and the reference layout of
reduce_cases.py (genomes of exactly 1, 63, 64, 65, 128, 129 and 3 bins), through ani_compute_cgi (one query), ani_reduce_check (several
queries in one table, with and without the gate), hand-made ties and losers, the gate's edges, 1, 2, 64 and 65 records per launch
(ANI_TEST_HITS_PIECE), the life cycle and the argument checks, with the profile and the distributions beside it, and end to end through
ani_map_cgi_batch, ani_map_cgi_fragset(s) and a merged set on small related genomes with a default engine, one of many sub-batches, a
chunked and a streamed reference set — once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu).
Every comparison is on bits."""
import numpy as np
import pytest

import hits_cases as hc
import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_profile import E2E_CONFIGS, ProfileWorld
from test_reducer import CONFIGS, MANY_CONFIGS

ONE_CASES = [("default", name) for name in hc.LISTS_ONE] + [(c, name) for c in CONFIGS if c != "default" for name in hc.LISTS_OTHER_CONFIGS]
ALL_MANY_CONFIGS = tuple(MANY_CONFIGS) + tuple(c for c in CONFIGS if c not in MANY_CONFIGS)      # default, chunked; streamed, id base
PIECES = (1, 2, 64, 65)


class HitsWorld(ProfileWorld):
    """... engines that take the records 1, 2, 64 and 65 per launch and copy, and the end-to-end inputs per fragment length"""

    def __init__(self, make_engine, default_engine, alloc):
        super().__init__(make_engine, default_engine)
        self.alloc = alloc
        self.e2es = {}

    def engine(self, config):
        if isinstance(config, tuple):
            if config not in self.engines:
                with pytest.MonkeyPatch.context() as mp:
                    self.engines[config] = self.make_engine(mp, ANI_TEST_HITS_PIECE=config[1])
            return self.engines[config]
        return super().engine(config)

    def hits_end_to_end(self, config, frag_len):
        if frag_len not in self.e2es:
            self.e2es[frag_len] = hc.EndToEnd(self.default_engine, frag_len)
        e2e = self.e2es[frag_len]
        if config == "default":
            return e2e, self.default_engine
        key = (config, frag_len)
        if key not in self.e2e_engines:
            env = dict(ANI_SUBBATCH_FRAGS=20)             # a few genomes per sub-batch, several sub-batches
            if config in ("chunked", "streamed"):
                env = dict(ANI_MAX_INDEX_MINIMIZERS=e2e.n_minimizers // 4)
            if config == "streamed":
                env["ANI_MAX_RESIDENT_CHUNKS"] = 1
            with pytest.MonkeyPatch.context() as mp:
                self.e2e_engines[key] = self.make_engine(mp, **env)
        return e2e, self.e2e_engines[key]


def _host_alloc(nbytes):
    a = np.zeros(nbytes // 4 + 4, dtype=np.uint32)
    return a, a.ctypes.data


def _device_alloc(nbytes):
    import torch
    t = torch.zeros(nbytes // 4 + 4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


# ---- the restatement against the oracle: CPU only, no engine ----
@pytest.mark.parametrize("name", hc.LISTS_RESTATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_restatement(frag_len, name):
    hc.case_restatement(frag_len, name)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = HitsWorld(_emu_engine_with, emu_engine, _host_alloc)
    yield w
    w.close()


@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_one_query(emu, config, frag_len, name):
    hc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_ties(emu, config, frag_len):
    hc.case_ties(emu.ref(config, frag_len))


@pytest.mark.parametrize("name", hc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ALL_MANY_CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    hc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", hc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate(emu, config, frag_len, name):
    hc.case_many(emu.ref(config, frag_len), name, gated=True)


@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_gate_edges(emu, config):
    hc.case_gate_edges(emu.ref(config, 1000))


@pytest.mark.parametrize("piece", PIECES)
def test_emu_pieces(emu, piece):
    hc.case_pieces(emu.ref(("piece", piece), 1000), piece)


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    hc.case_life_cycle(emu.ref(config, 1000))


def test_emu_arguments(emu, emu_engine):
    hc.case_arguments(emu.ref("default", 1000))
    hc.case_destroy_while_on(emu_engine)


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_together(emu, config):
    hc.case_together(emu.ref(config, 1000))


@pytest.mark.parametrize("frag_len", hc.E2E_FRAG_LENS)
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_emu_end_to_end(emu, config, frag_len):
    e2e, engine = emu.hits_end_to_end(config, frag_len)
    e2e.run(engine, config, emu.alloc)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = HitsWorld(_engine_with, gpu_engine, _device_alloc)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_one_query(gpu, config, frag_len, name):
    hc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_ties(gpu, config, frag_len):
    hc.case_ties(gpu.ref(config, frag_len))


@pytest.mark.gpu
@pytest.mark.parametrize("name", hc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ALL_MANY_CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    hc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", hc.LISTS_GATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate(gpu, config, frag_len, name):
    hc.case_many(gpu.ref(config, frag_len), name, gated=True)


@pytest.mark.gpu
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_gate_edges(gpu, config):
    hc.case_gate_edges(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("piece", PIECES)
def test_gpu_pieces(gpu, piece):
    hc.case_pieces(gpu.ref(("piece", piece), 1000), piece)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    hc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_arguments(gpu, gpu_engine):
    hc.case_arguments(gpu.ref("default", 1000))
    hc.case_destroy_while_on(gpu_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_together(gpu, config):
    hc.case_together(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", hc.E2E_FRAG_LENS)
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_gpu_end_to_end(gpu, config, frag_len):
    e2e, engine = gpu.hits_end_to_end(config, frag_len)
    e2e.run(engine, config, gpu.alloc)


# ---- the command line ----
CLI_CASES = ((3000, True), (1500, False))


@pytest.mark.parametrize("frag_len,full", CLI_CASES)
def test_emu_cli(emu_engine, tmp_path, frag_len, full):
    import os
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir, "all"])
    hc.case_cli(os.path.join(emu_dir, "fastANI_emu"), emu_engine, str(tmp_path), frag_len, full)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len,full", CLI_CASES)
def test_gpu_cli(gpu_engine, tmp_path, frag_len, full):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hc.case_cli(os.path.join(root, "fastani_amd", "fastANI"), gpu_engine, str(tmp_path), frag_len, full)
