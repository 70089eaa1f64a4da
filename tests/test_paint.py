"""The paint records — every query fragment's best reference over the whole reference set (kernels/paint.hpp: k_paint_best, k_paint_second,
k_paint_flags and k_paint_records, launched by reduce_stage; the ani_sketch_paint_* calls and ani_paint_merge of engine_map.hip; --paint
of the command line) against the numpy restatement of their rules in paint_cases.py — whose 1-way winners are first held to the oracle's
rows on the CPU alone — on the synthetic lists and the reference layout of reduce_cases.py (genomes of exactly 1, 63, 64, 65, 128, 129
and 3 bins), through ani_compute_cgi (one query) and ani_reduce_check (several queries in one table, a non-zero genomeBase) under every
engine configuration of test_reducer.py, hand-made lists, 1, 2, 64 and 65 records per launch (ANI_TEST_PAINT_PIECE), ani_paint_merge on
its own, the life cycle and the argument checks, the other four record modes beside it, and end to end through ani_map_cgi_batch,
ani_map_cgi_fragset(s) and a merged set on small related genomes with a default engine, one of many sub-batches, a chunked and a streamed
reference set — once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu).  Every comparison is on
bits."""
import numpy as np
import pytest

import paint_cases as ptc
import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_hits import _device_alloc, _host_alloc
from test_profile import E2E_CONFIGS, ProfileWorld
from test_reducer import CONFIGS

ONE_CASES = [("default", name) for name in ptc.LISTS_ONE] + [(c, name) for c in CONFIGS if c != "default" for name in ptc.LISTS_OTHER_CONFIGS]
PIECES = (1, 2, 64, 65)
E2E_CASES = [(c, ptc.E2E_FRAG_LENS[0]) for c in E2E_CONFIGS] + [("default", L) for L in ptc.E2E_FRAG_LENS[1:]]      # every engine, and a second fragment length


class PaintWorld(ProfileWorld):
    """... engines that take the records 1, 2, 64 and 65 per launch and copy, the 70-genome set, and the end-to-end inputs per fragment
    length"""

    def __init__(self, make_engine, default_engine, alloc):
        super().__init__(make_engine, default_engine)
        self.alloc = alloc
        self.e2es = {}
        self.many = {}

    def engine(self, config):
        if isinstance(config, tuple):
            if config not in self.engines:
                with pytest.MonkeyPatch.context() as mp:
                    self.engines[config] = self.make_engine(mp, ANI_TEST_PAINT_PIECE=config[1])
            return self.engines[config]
        return super().engine(config)

    def many_genomes(self, config):
        if config not in self.many:
            if config == "default":
                self.many[config] = ptc.ManyGenomes(self.default_engine)
            else:
                n = self.many_genomes("default").sk.stats()["minimizers"]
                with pytest.MonkeyPatch.context() as mp:
                    self.engines["many", config] = self.make_engine(mp, ANI_MAX_INDEX_MINIMIZERS=max(n // 4, 1))
                self.many[config] = ptc.ManyGenomes(self.engines["many", config])
                assert len(self.many[config].sk.chunks()) >= 3, self.many[config].sk.chunks()
        return self.many[config]

    def paint_end_to_end(self, config, frag_len):
        if frag_len not in self.e2es:
            self.e2es[frag_len] = ptc.EndToEnd(self.default_engine, frag_len)
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

    def close(self):
        for m in self.many.values():
            m.close()
        super().close()


# ---- the restatement against the oracle: CPU only, no engine ----
@pytest.mark.parametrize("name", ptc.LISTS_RESTATE)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_restatement(frag_len, name):
    ptc.case_restatement(frag_len, name)


# ---- ani_paint_merge: a host function, the CPU build's ----
def test_merge(emu_engine):
    ptc.case_merge(emu_engine.lib)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = PaintWorld(_emu_engine_with, emu_engine, _host_alloc)
    yield w
    w.close()


@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_one_query(emu, config, frag_len, name):
    ptc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", ptc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    ptc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_hand_made(emu, config, frag_len):
    ptc.case_hand_made(emu.ref(config, frag_len))


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_block_border(emu, config):
    ptc.case_block_border(emu.ref(config, 1000))


@pytest.mark.parametrize("n", (255, 256, 257))
@pytest.mark.parametrize("config", ("default", "chunked", "streamed"))
def test_emu_scan_border(emu, config, n):
    ptc.case_scan_border(emu.ref(config, 1000), n)


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_many_genomes(emu, config):
    ptc.case_many_genomes(emu.many_genomes(config))


@pytest.mark.parametrize("piece", PIECES)
def test_emu_pieces(emu, piece):
    ptc.case_pieces(emu.ref(("piece", piece), 1000), piece)


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    ptc.case_life_cycle(emu.ref(config, 1000))


def test_emu_arguments(emu, emu_engine):
    ptc.case_arguments(emu.ref("default", 1000))
    ptc.case_destroy_while_on(emu_engine)


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_together(emu, config):
    ptc.case_together(emu.ref(config, 1000))


@pytest.mark.parametrize("config,frag_len", E2E_CASES)
def test_emu_end_to_end(emu, config, frag_len):
    e2e, engine = emu.paint_end_to_end(config, frag_len)
    e2e.run(engine, config, emu.alloc)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = PaintWorld(_engine_with, gpu_engine, _device_alloc)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_one_query(gpu, config, frag_len, name):
    ptc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ptc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    ptc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_hand_made(gpu, config, frag_len):
    ptc.case_hand_made(gpu.ref(config, frag_len))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_block_border(gpu, config):
    ptc.case_block_border(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (255, 256, 257))
@pytest.mark.parametrize("config", ("default", "chunked", "streamed"))
def test_gpu_scan_border(gpu, config, n):
    ptc.case_scan_border(gpu.ref(config, 1000), n)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_many_genomes(gpu, config):
    ptc.case_many_genomes(gpu.many_genomes(config))


@pytest.mark.gpu
@pytest.mark.parametrize("piece", PIECES)
def test_gpu_pieces(gpu, piece):
    ptc.case_pieces(gpu.ref(("piece", piece), 1000), piece)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    ptc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_arguments(gpu, gpu_engine):
    ptc.case_arguments(gpu.ref("default", 1000))
    ptc.case_destroy_while_on(gpu_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_together(gpu, config):
    ptc.case_together(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("config,frag_len", E2E_CASES)
def test_gpu_end_to_end(gpu, config, frag_len):
    e2e, engine = gpu.paint_end_to_end(config, frag_len)
    e2e.run(engine, config, gpu.alloc)


# ---- the command line ----
def test_emu_cli(emu_engine, tmp_path):
    import os
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir, "all"])
    ptc.case_cli(os.path.join(emu_dir, "fastANI_emu"), emu_engine, str(tmp_path), 3000)


@pytest.mark.gpu
def test_gpu_cli(gpu_engine, tmp_path):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ptc.case_cli(os.path.join(root, "fastani_amd", "fastANI"), gpu_engine, str(tmp_path), 3000)
