"""The synteny records (kernels/synteny.hpp: k_syn_list, k_syn_pairs and k_syn_compact, launched by reduce_stage; the
ani_sketch_synteny_* calls of engine_map.hip; --synteny of the command line) against the numpy restatement of their rules in
synteny_cases.py: hand-made lists whose answers are written out (n = 1 and 2, identity, reversal, inversion, translocation, alternating
order, a reference contig border, unmatched fragments between matched ones, querySeqIds 0 and 2^31 - 1), the synthetic lists and the
reference layout of reduce_cases.py (genomes of exactly 1, 63, 64, 65, 128, 129 and 3 bins) through ani_compute_cgi and
ani_reduce_check under every engine configuration, pairs of 1, 2, 31 .. 33, 63 .. 65 and 255 .. 257 hits, the device-pool path beside
the LDS path (ANI_TEST_SYNTENY_LDS_HITS=32), 1, 2, 64 and 65 pairs per launch (ANI_TEST_SYNTENY_PIECE), the gate's edges and a gate that
differs from the hits' in one call, the life cycle and the argument checks, the invariants against --ci, and end to end on small related
genomes with a default engine, one of many sub-batches, a chunked and a streamed reference set — once on the CPU-emulation build (not
gpu) and once on the product library on an MI355X (gpu).  In every engine case the hits are on beside the synteny records, and the
synteny records equal the restatement of the hits the same call returned, byte for byte."""
import pytest

import hits_cases as hc
import reduce_cases as rc
import synteny_cases as sc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_hits import _device_alloc, _host_alloc
from test_profile import E2E_CONFIGS, ProfileWorld
from test_reducer import CONFIGS

ONE_CASES = [("default", name) for name in hc.LISTS_ONE] + [(c, name) for c in CONFIGS if c != "default" for name in hc.LISTS_OTHER_CONFIGS]
PIECES = (1, 2, 64, 65)
LDS_CAP = 32


class SyntenyWorld(ProfileWorld):
    """... engines that take 1, 2, 64 and 65 pairs per launch or keep 32 hits of a pair in LDS, the reference with a 300-bin genome per
    engine, and the end-to-end inputs per fragment length"""

    def __init__(self, make_engine, default_engine, alloc):
        super().__init__(make_engine, default_engine)
        self.alloc = alloc
        self.e2es, self.bigs = {}, {}

    def engine(self, config):
        if isinstance(config, tuple):
            if config not in self.engines:
                with pytest.MonkeyPatch.context() as mp:
                    self.engines[config] = self.make_engine(mp, **{config[0]: config[1]})
            return self.engines[config]
        return super().engine(config)

    def big(self, config):
        if config not in self.bigs:
            self.bigs[config] = sc.BigRef(self.engine(config))
        return self.bigs[config]

    def synteny_end_to_end(self, config, frag_len):
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

    def close(self):
        for b in self.bigs.values():
            b.close()
        super().close()


# ---- the restatement against the answers written out: CPU only, no engine ----
@pytest.mark.parametrize("name", sorted(sc.HAND))
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_restatement(frag_len, name):
    sc.case_restatement(frag_len, name)


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = SyntenyWorld(_emu_engine_with, emu_engine, _host_alloc)
    yield w
    w.close()


@pytest.mark.parametrize("name", sorted(sc.HAND))
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_hand(emu, config, frag_len, name):
    sc.case_hand(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_one_query(emu, config, frag_len, name):
    sc.case_one_query(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", hc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    sc.case_many(emu.ref(config, frag_len), name)


@pytest.mark.parametrize("name", hc.LISTS_GATE)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_gate(emu, config, name):
    sc.case_many(emu.ref(config, 1000), name, gated=True)


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_gate_edges(emu, config):
    sc.case_gate_edges(emu.ref(config, 1000))


def test_emu_sizes(emu):
    sc.case_sizes(emu.big("default"))


def test_emu_sizes_pool(emu):
    sc.case_sizes(emu.big(("ANI_TEST_SYNTENY_LDS_HITS", LDS_CAP)), LDS_CAP)


@pytest.mark.parametrize("piece", PIECES)
def test_emu_pieces(emu, piece):
    sc.case_pieces(emu.ref(("ANI_TEST_SYNTENY_PIECE", piece), 1000), piece)


@pytest.mark.parametrize("config", ("default", "streamed"))
def test_emu_life_cycle(emu, config):
    sc.case_life_cycle(emu.ref(config, 1000))


def test_emu_arguments(emu, emu_engine):
    sc.case_arguments(emu.ref("default", 1000))
    sc.case_destroy_while_on(emu_engine)


@pytest.mark.parametrize("config", ("default", "chunked"))
def test_emu_together(emu, config):
    sc.case_together(emu.ref(config, 1000))


@pytest.mark.parametrize("frag_len", hc.E2E_FRAG_LENS[:1])               # (the mapper on the CPU stand-in is slow: both lengths on the device)
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_emu_end_to_end(emu, config, frag_len):
    e2e, engine = emu.synteny_end_to_end(config, frag_len)
    sc.e2e_run(e2e, engine, config, emu.alloc)


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = SyntenyWorld(_engine_with, gpu_engine, _device_alloc)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sc.HAND))
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_hand(gpu, config, frag_len, name):
    sc.case_hand(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("config,name", ONE_CASES)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_one_query(gpu, config, frag_len, name):
    sc.case_one_query(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", hc.LISTS_MANY)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    sc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", hc.LISTS_GATE)
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_gate(gpu, config, name):
    sc.case_many(gpu.ref(config, 1000), name, gated=True)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_gate_edges(gpu, config):
    sc.case_gate_edges(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_sizes(gpu):
    sc.case_sizes(gpu.big("default"))


@pytest.mark.gpu
def test_gpu_sizes_pool(gpu):
    sc.case_sizes(gpu.big(("ANI_TEST_SYNTENY_LDS_HITS", LDS_CAP)), LDS_CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("piece", PIECES)
def test_gpu_pieces(gpu, piece):
    sc.case_pieces(gpu.ref(("ANI_TEST_SYNTENY_PIECE", piece), 1000), piece)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "streamed"))
def test_gpu_life_cycle(gpu, config):
    sc.case_life_cycle(gpu.ref(config, 1000))


@pytest.mark.gpu
def test_gpu_arguments(gpu, gpu_engine):
    sc.case_arguments(gpu.ref("default", 1000))
    sc.case_destroy_while_on(gpu_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "chunked"))
def test_gpu_together(gpu, config):
    sc.case_together(gpu.ref(config, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", hc.E2E_FRAG_LENS)
@pytest.mark.parametrize("config", E2E_CONFIGS)
def test_gpu_end_to_end(gpu, config, frag_len):
    e2e, engine = gpu.synteny_end_to_end(config, frag_len)
    sc.e2e_run(e2e, engine, config, gpu.alloc)


# ---- the command line ----
def test_emu_cli(emu_engine, tmp_path):
    import os
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir, "all"])
    sc.case_cli(os.path.join(emu_dir, "fastANI_emu"), emu_engine, str(tmp_path), 3000)


@pytest.mark.gpu
def test_gpu_cli(gpu_engine, tmp_path):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sc.case_cli(os.path.join(root, "fastani_amd", "fastANI"), gpu_engine, str(tmp_path), 3000)
