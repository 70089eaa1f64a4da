"""The L2 stage — sliding MinHash over a candidate's range, kernels/l2.hpp behind l2_stage (the second half of map_stage,
engine_map.hip): k_l2_ranges, the length ordering, k_l2_codes, k_l2_sim<A> / <B>, the collection kernels, k_l2, k_finish_candidates —
on synthetic index records and hand-written fragment sketches, candidates to placement: the nine arrays of one call (the ordered
candidates, l2Best, l2First, l2Last, refStart, idBits) and the increase of the L2 counters held to the from-scratch definition of
computeL2MappedRegions (l2_cases.py) — once on the CPU-emulation build (not gpu) and once on the product library on an MI355X (gpu),
through the test entry point ani_l2_check.

Every family runs through the fast path, through the general kernel (ANI_TEST_L2_PATH=general) and through class B (classB); the fast
path and the general kernel must also agree with each other on every word and on l2Steps, l2WindowEntries and l2QueryHashes.  Each
case first asserts, from the definition alone, that its input reaches the edge it names (routing counts, ties, best == 0).  Every
comparison is exact.  test_definition_forms (CPU only) holds the literal incremental form of slidingMap.hpp to the from-scratch count
on every case."""
import pytest

import l2_cases as l2
from test_index_build import emu, gpu      # noqa: F401  (the two halves' World: engines and memory)

GAPS = [(c, wh, nb) for c in l2.GAP_COUNTS for wh in l2.GAP_WHERE for nb in (0, 1)]
GEOMETRY = ((16, 3000), (12, 1000))
TOP = [(c, wh, ff) for c in l2.TOP_COUNTS for wh in l2.TOP_WHERE for ff in (0, 1)]
RANK = [(w, ff) for w in l2.RANK_WINDOWS for ff in (0, 1)]


@pytest.mark.parametrize("family", l2.FAMILIES)
def test_definition_forms(family):
    l2.case_definition_forms(family)


# ---- the CPU-emulation build ----
@pytest.mark.parametrize("s", l2.SKETCH_SIZES)
def test_emu_sketch_size(emu, s):
    l2.case_sketch_size(emu, s)


@pytest.mark.parametrize("s", l2.GEOMETRY_SIZES)
def test_emu_sketch_size_geometry(emu, s):
    l2.case_sketch_size(emu, s, k=12, L=1000)


@pytest.mark.parametrize("entries", l2.RANGE_LENGTHS)
def test_emu_range_length(emu, entries):
    l2.case_range_length(emu, entries)


@pytest.mark.parametrize("count,where,neighbour", GAPS)
def test_emu_gap_counter(emu, count, where, neighbour):
    l2.case_gap_counter(emu, count, where, neighbour)


@pytest.mark.parametrize("count,where,ff", TOP)
def test_emu_gap_counter_top(emu, count, where, ff):
    l2.case_gap_counter_top(emu, count, where, ff)


@pytest.mark.parametrize("k,frag_len", GEOMETRY)
def test_emu_window_shapes(emu, k, frag_len):
    l2.case_window_shapes(emu, k, frag_len)


@pytest.mark.parametrize("k,frag_len", GEOMETRY)
def test_emu_same_hash(emu, k, frag_len):
    l2.case_same_hash(emu, k, frag_len)


@pytest.mark.parametrize("w,ff_in_sketch", RANK)
def test_emu_rank_table(emu, w, ff_in_sketch):
    l2.case_rank_table(emu, w, ff_in_sketch)


@pytest.mark.parametrize("n_cand", l2.MANY)
def test_emu_many_candidates(emu, n_cand):
    l2.case_many(emu, n_cand)


@pytest.mark.parametrize("events", l2.STREAMS)
def test_emu_stream_length(emu, events):
    l2.case_stream(emu, events)


def test_emu_arguments(emu):
    l2.case_arguments(emu)


# ---- the product library on the device ----
@pytest.mark.gpu
@pytest.mark.parametrize("s", l2.SKETCH_SIZES)
def test_gpu_sketch_size(gpu, s):
    l2.case_sketch_size(gpu, s)


@pytest.mark.gpu
@pytest.mark.parametrize("s", l2.GEOMETRY_SIZES)
def test_gpu_sketch_size_geometry(gpu, s):
    l2.case_sketch_size(gpu, s, k=12, L=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", l2.RANGE_LENGTHS)
def test_gpu_range_length(gpu, entries):
    l2.case_range_length(gpu, entries)


@pytest.mark.gpu
@pytest.mark.parametrize("count,where,neighbour", GAPS)
def test_gpu_gap_counter(gpu, count, where, neighbour):
    l2.case_gap_counter(gpu, count, where, neighbour)


@pytest.mark.gpu
@pytest.mark.parametrize("count,where,ff", TOP)
def test_gpu_gap_counter_top(gpu, count, where, ff):
    l2.case_gap_counter_top(gpu, count, where, ff)


@pytest.mark.gpu
@pytest.mark.parametrize("k,frag_len", GEOMETRY)
def test_gpu_window_shapes(gpu, k, frag_len):
    l2.case_window_shapes(gpu, k, frag_len)


@pytest.mark.gpu
@pytest.mark.parametrize("k,frag_len", GEOMETRY)
def test_gpu_same_hash(gpu, k, frag_len):
    l2.case_same_hash(gpu, k, frag_len)


@pytest.mark.gpu
@pytest.mark.parametrize("w,ff_in_sketch", RANK)
def test_gpu_rank_table(gpu, w, ff_in_sketch):
    l2.case_rank_table(gpu, w, ff_in_sketch)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand", l2.MANY)
def test_gpu_many_candidates(gpu, n_cand):
    l2.case_many(gpu, n_cand)


@pytest.mark.gpu
@pytest.mark.parametrize("events", l2.STREAMS)
def test_gpu_stream_length(gpu, events):
    l2.case_stream(gpu, events)


@pytest.mark.gpu
def test_gpu_arguments(gpu):
    l2.case_arguments(gpu)
