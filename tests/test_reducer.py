"""The ANI reducer (kernels/reduce.hpp: k_oneway_bins and k_pair_reduce, driven by ani_compute_cgi, reduce_stage and collect_rows of
engine_map.hip) on synthetic mapping lists against the oracle's sort-and-dedup form of computeCGI: the cases of reduce_cases.py — a
reference layout whose genomes have exactly 1, 63, 64, 65, 128, 129 and 3 bins, lists that sit on the tie-break, the bin edges, the
64-bin slab edge, the summation order and the launch-block borders, every list in order and shuffled, against the default engine, a
chunked and a streamed reference set and a sketch with a reference id base — once on the CPU-emulation build (not gpu) and once on
the product library on an MI355X (gpu).  ani_reduce_check (test infrastructure, engine_map.hip) gives the reducer the shape of the
fused path: several queries in one table, a non-zero genomeBase, a partial last workgroup of the pair grid.

Only the GPU half sees the device forms — __ballot / readlane in bin order, atomicMax on the identity bits, the grid's early return —
which the CPU stand-in replaces with plain code.  Rows are compared bit for bit; there is no tolerance."""
import pytest

import reduce_cases as rc
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with

CONFIGS = ("default", "chunked", "streamed", "ref_id_base")
MANY_CONFIGS = ("default", "chunked")


class World:
    """the engines and reference sets of one half (emulation or device), made when a test first asks for them and kept for the module"""

    def __init__(self, make_engine, default_engine):
        self.make_engine, self.default_engine = make_engine, default_engine
        self.engines, self.refs = {}, {}

    def engine(self, config):
        if config in ("default", "ref_id_base"):
            return self.default_engine
        if config not in self.engines:
            # a limit that cuts the smaller of the two layouts' sketches into four or more index chunks
            w = {L: self.default_engine.params(rc.K, L).windowSize for L in rc.FRAG_LENS}
            env = dict(ANI_MAX_INDEX_MINIMIZERS=min(rc.minimizer_count(L, w[L]) for L in rc.FRAG_LENS) // 4)
            if config == "streamed":
                env["ANI_MAX_RESIDENT_CHUNKS"] = 1
            with pytest.MonkeyPatch.context() as mp:      # the engine reads its environment when it is made
                self.engines[config] = self.make_engine(mp, **env)
        return self.engines[config]

    def ref(self, config, frag_len):
        if (config, frag_len) not in self.refs:
            ref = rc.Ref(self.engine(config), frag_len, ref_id_base=1000 if config == "ref_id_base" else 0)
            if config in ("chunked", "streamed"):
                # one fragment's mappings reach genomes in different chunks
                assert len(ref.sk.chunks()) >= 3 and ref.sk.chunks()[0] == 0, ref.sk.chunks()
                assert ref.sk.residency()["streaming"] == (config == "streamed")
            else:
                assert len(ref.sk.chunks()) == 1
            self.refs[config, frag_len] = ref
        return self.refs[config, frag_len]

    def close(self):
        for ref in self.refs.values():
            ref.close()
        for e in self.engines.values():
            e.close()


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_layout(frag_len):
    """the bin totals and the contig lengths around k * binW, from the contig lengths: a change to the layout cannot drop the edges"""
    rc.check_layout(rc.Layout(frag_len))


# ---- the CPU-emulation build ----
@pytest.fixture(scope="module")
def emu(emu_engine):
    w = World(_emu_engine_with, emu_engine)
    yield w
    w.close()


@pytest.mark.parametrize("name", sorted(rc.LISTS))
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_list(emu, config, frag_len, name):
    rc.case_list(emu.ref(config, frag_len), name, runs=3 if name == "hot_bin" else 1)


@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_emu_arguments(emu, frag_len):
    rc.case_arguments(emu.ref("default", frag_len))


@pytest.mark.parametrize("name", rc.MANY_LISTS)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_emu_many_queries(emu, config, frag_len, name):
    rc.case_many(emu.ref(config, frag_len), name)


def test_emu_many_queries_arguments(emu):
    rc.case_many_arguments(emu.ref("default", 1000))


# ---- the product library on the device ----
@pytest.fixture(scope="module")
def gpu(gpu_engine):
    w = World(_engine_with, gpu_engine)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rc.LISTS))
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gpu_list(gpu, config, frag_len, name):
    rc.case_list(gpu.ref(config, frag_len), name, runs=3 if name == "hot_bin" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
def test_gpu_arguments(gpu, frag_len):
    rc.case_arguments(gpu.ref("default", frag_len))


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.MANY_LISTS)
@pytest.mark.parametrize("frag_len", rc.FRAG_LENS)
@pytest.mark.parametrize("config", MANY_CONFIGS)
def test_gpu_many_queries(gpu, config, frag_len, name):
    rc.case_many(gpu.ref(config, frag_len), name)


@pytest.mark.gpu
def test_gpu_many_queries_arguments(gpu):
    rc.case_many_arguments(gpu.ref("default", 1000))
