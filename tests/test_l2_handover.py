"""The first super-window of an L2 candidate reaches k_l2_sim as state, not as events (kernels/l2.hpp: k_l2_codes sums the inserts
of the entries [beg0, end0 - 1) in a per-wave histogram and writes the packed fields in front of the event stream; k_l2_sim loads
them and finds the pivot on the way).  Every case compares mappings and rows with the CPU oracle, bit for bit; the emulator
tests run the same sources on the CPU (tests/emu), their `gpu` twins the product library.

What the inputs cover:
  case_tandem_repeats        same-hash entries inside the first window (the histogram must skip them as the sliding map's set
                             does) and a 21-kb candidate whose stream is longer than the wave's LDS stage window
  case_gap_counter_overflow  a field beyond 255 while the first window fills: k_l2_codes sends the candidate to the general kernel
  window sizes 19..22        s = 270..300: class B, and a first window that crosses the 256-entry pass of k_l2_codes; with a 600-base
                             N run in every query fragment: s <= 255 (class A) against first windows of more than 256 entries
  fragments of 500 bases,    first windows of exactly ONE entry, i.e. an empty state handed over: with window size 300 a super-window
  window size 300            spans 500 - 299 - 15 = 186 positions, less than the usual distance between two minimizers (the five
                             cases above have no such candidate: at the default parameters a super-window holds ~240 entries).
                             Seen once on the emulator, with a print in k_l2_ranges while this file was written: at least 6 of
                             the input's 23 candidates start with a one-entry window (s = 1..3, ranges of 5..7 entries)
under the knobs that move chunk borders (ANI_TEST_L2_CHUNK=13), send everything through class B (ANI_TEST_L2_PATH=classB) and halve
chunks whose code stream passes the offset limit (ANI_TEST_L2_CODE_LIMIT=6000 with chunks of 64)."""
import ctypes
import os

import numpy as np
import pytest

import orc
import parity_cases as pc
from fastani_amd.api import Engine, Sketch

KNOBS = [dict(ANI_TEST_L2_CHUNK=13), dict(ANI_TEST_L2_PATH="classB"), dict(ANI_TEST_L2_CODE_LIMIT=6000, ANI_TEST_L2_CHUNK=64)]
KNOB_IDS = ["chunk13", "classB", "codeLimit6000"]


def _synthetic_cluster(e):
    pc.case_synthetic_cluster(e, 30000)


CASES = [_synthetic_cluster, pc.case_tandem_repeats, pc.case_gap_counter_overflow, pc.case_messy, pc.case_low_complexity]
CASE_IDS = ["synthetic_cluster", "tandem_repeats", "gap_counter_overflow", "messy", "low_complexity"]


def _emu(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    here = os.path.dirname(os.path.abspath(__file__))
    return Engine(ctypes.CDLL(os.path.join(here, "emu", "libfastani_emu.so")), 0)


def _gpu(monkeypatch, **env):
    from fastani_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return Engine(_lib.load(), 0)


def _run_case(e, case):
    e.reset_counters()
    case(e)                                   # case_gap_counter_overflow asserts l2SlowOverflow > 0 itself
    c = e.counters()
    assert c["l2FastCandidates"] > 0, c
    e.close()


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emu_cases(emu_engine, monkeypatch, case, knobs):
    _run_case(_emu(monkeypatch, **knobs), case)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_cases(gpu_engine, monkeypatch, case, knobs):
    _run_case(_gpu(monkeypatch, **knobs), case)


def _window_case_with_n_runs(e, windows=(19, 20, 21, 22)):
    """references sketched with windows 19..22 (~270-300 minimizers per 3 kb: first windows beyond one 256-entry pass), queries whose
    fragments each carry a 600-base N run (s <= 255: class A), against the oracle"""
    ref = orc.synth_genome(6, 0, 30000)
    qry = pc.mutate(ref, 0.03, 11)
    for f in range(len(qry) // 3000):
        qry[f * 3000 + 1200:f * 3000 + 1800] = ord("N")
    genomes = [[ref], [orc.synth_genome(6, 2, 9000)]]
    e.reset_counters()
    for w in windows:
        p = e.params(16, 3000)
        p.windowSize = w
        sk = Sketch(e, p, genomes)
        osk = orc.Sketch(genomes, 16, w)
        fr = e.query_sketch(p, [[qry]])
        assert len(fr) == 10 and max(len(x) for x in fr) <= 255, [len(x) for x in fr]
        maps, tot = sk.map_query([qry])
        omaps, otot = osk.map_genome([qry], 3000)
        assert tot == otot and len(maps) == len(omaps) >= 8, (w, len(maps), len(omaps))
        assert np.array_equal(maps, omaps), w
        assert np.array_equal(sk.compute_cgi(maps, tot, 0), osk.compute_cgi(omaps, otot, 0, 3000)), w
        sk.close()
    c = e.counters()
    assert c["l2FastCandidates"] > 0 and c["l2SlowCandidates"] == 0, c


def _one_entry_first_windows(e):
    """500-base fragments, window size 300: candidates whose first super-window is its first entry alone (see the module docstring)"""
    ref = pc.rng_genome(41, 12000)
    qry = pc.mutate(ref, 0.02, 42)
    genomes = [[ref], [pc.rng_genome(43, 6000)]]
    p = e.params(16, 500)
    p.windowSize = 300
    sk = Sketch(e, p, genomes)
    osk = orc.Sketch(genomes, 16, 300)
    e.reset_counters()
    maps, tot = sk.map_query([qry])
    omaps, otot = osk.map_genome([qry], 500)
    assert tot == otot and len(maps) == len(omaps) >= 20, (len(maps), len(omaps))
    assert np.array_equal(maps, omaps)
    assert np.array_equal(sk.compute_cgi(maps, tot, 0), osk.compute_cgi(omaps, otot, 0, 500))
    c = e.counters()
    assert c["l2FastCandidates"] >= 20 and c["l2SlowCandidates"] == 0, c
    sk.close()


def test_emu_one_entry_first_windows(emu_engine):
    _one_entry_first_windows(emu_engine)


@pytest.mark.gpu
def test_gpu_one_entry_first_windows(gpu_engine):
    _one_entry_first_windows(gpu_engine)


def test_emu_window_sizes(emu_engine):
    pc.case_window_sizes(emu_engine, windows=(19, 20, 21, 22))


def test_emu_window_sizes_n_runs(emu_engine):
    _window_case_with_n_runs(emu_engine)


@pytest.mark.gpu
def test_gpu_window_sizes(gpu_engine):
    pc.case_window_sizes(gpu_engine, windows=(19, 20, 21, 22))


@pytest.mark.gpu
def test_gpu_window_sizes_n_runs(gpu_engine):
    _window_case_with_n_runs(gpu_engine)
