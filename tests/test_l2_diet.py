"""k_l2_sim tracks its result in two packed keys and counts what it evaluated once per block (kernels/l2.hpp: run_block), and
l2_apply decides the pivot's move from one comparison alone.  Every case compares mappings and rows with the CPU oracle, bit for
bit; the emulator tests run the same sources on the CPU (tests/emu), their `gpu` twins the product library.

What the inputs cover, and what of the changed code they reach:
  case_tandem_repeats     a 700-base tandem repeat: many windows tie for the best shared count, so the first and the last position
                          at the best differ (keyFirst / keyLast unpack to different entries); same-hash neighbours flagged nearDup
  case_low_complexity     near-duplicate entries throughout: the blocks take the general form and delCount is read mid-block by the
                          same-hash look-ups
  fragments of 500 bases, streams of fewer than 8 events and of lengths that are no multiple of 8 (ranges of 5..7 entries, s = 1..3): the
  window size 300         partial last block takes the general form, where the evaluated events are counted under the mask of the lane's
                          remaining events.  The queries are mutated at 2, 5 and 8 %: with s = 1..3 a candidate's only shared hash is
                          sometimes not among the s smallest of any window, so its best stays 0, the first position stays unset and
                          the last one is that of the last evaluation.  Seen once on the emulator, with a print at the end of
                          k_l2_sim while this file was written: see the figures in _short_streams
  case_synthetic_cluster  ordinary candidates (~240 entries per window), plain blocks
under no knob, under ANI_TEST_L2_CHUNK=13 (chunk borders that leave waves with lanes without a candidate: those lanes run as plain
with a sketch size of 0) and under ANI_TEST_L2_PATH=classB (everything through L2Geom<319>).

test_*_fast_path_against_general runs one input through the fast path and through ANI_TEST_L2_PATH=general and asserts equal
mappings and equal counters of evaluated placements (l2Steps), window entries and query hashes: the general kernel counts a
placement where it evaluates it, in code this change does not touch, so the per-block count of k_l2_sim is pinned against it."""
import ctypes
import os

import numpy as np
import pytest

import orc
import parity_cases as pc
from fastani_amd.api import Engine, Sketch

KNOBS = [dict(), dict(ANI_TEST_L2_CHUNK=13), dict(ANI_TEST_L2_PATH="classB")]
KNOB_IDS = ["plain", "chunk13", "classB"]


def _synthetic_cluster(e):
    pc.case_synthetic_cluster(e, 30000)


def _short_inputs():
    ref = pc.rng_genome(51, 12000)
    genomes = [[ref], [pc.rng_genome(53, 6000)]]
    return genomes, [pc.mutate(ref, 0.02, 52), pc.mutate(ref, 0.05, 54), pc.mutate(ref, 0.08, 54)]


def _short_streams(e):
    """500-base fragments, window size 300 (see the module docstring).  On the emulator, default knobs, k_l2_sim finished
    48 candidates on this input: all with fewer than 16 events, 25 of them with fewer than 8, 40 with a count that is no multiple of 8,
    30 whose first and last position at the best differ, and 3 whose best stayed 0 (each with the last position set)."""
    genomes, queries = _short_inputs()
    p = e.params(16, 500)
    p.windowSize = 300
    sk = Sketch(e, p, genomes)
    osk = orc.Sketch(genomes, 16, 300)
    e.reset_counters()
    n = 0
    for qi, q in enumerate(queries):
        maps, tot = sk.map_query([q])
        omaps, otot = osk.map_genome([q], 500)
        assert tot == otot and len(maps) == len(omaps), (qi, len(maps), len(omaps))
        assert np.array_equal(maps, omaps), qi
        assert np.array_equal(sk.compute_cgi(maps, tot, qi), osk.compute_cgi(omaps, otot, qi, 500)), qi
        n += len(maps)
    assert n >= 20, n
    c = e.counters()
    assert c["l2FastCandidates"] >= 20 and c["l2SlowCandidates"] == 0, c
    sk.close()


CASES = [_synthetic_cluster, pc.case_tandem_repeats, pc.case_low_complexity, _short_streams]
CASE_IDS = ["synthetic_cluster", "tandem_repeats", "low_complexity", "short_streams"]


def _set_env(monkeypatch, env):
    for k in ("ANI_TEST_L2_CHUNK", "ANI_TEST_L2_PATH", "ANI_TEST_L2_CODE_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _emu(monkeypatch, **env):
    _set_env(monkeypatch, env)
    here = os.path.dirname(os.path.abspath(__file__))
    return Engine(ctypes.CDLL(os.path.join(here, "emu", "libfastani_emu.so")), 0)


def _gpu(monkeypatch, **env):
    from fastani_amd import _lib
    _set_env(monkeypatch, env)
    return Engine(_lib.load(), 0)


def _run_case(e, case):
    e.reset_counters()
    case(e)
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


def _map_all(e):
    """mappings and L2 counters of three inputs: tandem repeats (3000-base fragments), near-duplicate entries, short streams"""
    out = []
    e.reset_counters()
    unit = pc.rng_genome(4, 700)
    rep = np.tile(unit, 30)
    flank = pc.rng_genome(6, 20000)
    ref = np.concatenate([flank[:10000], rep, flank[10000:]])
    qry = np.concatenate([flank[:10000], pc.mutate(rep, 0.03, 8), flank[10000:]])
    sk = Sketch(e, e.params(16, 3000), [[ref], [qry]])
    for q in ([qry], [ref]):
        out.append(sk.map_query(q)[0])
    sk.close()

    def runs(na, n):
        return np.frombuffer((b"A" * na + b"T") * (n // (na + 1) + 1), dtype=np.uint8)[:n]
    sk = Sketch(e, e.params(16, 3000), [[runs(64, 3500)], [runs(128, 3300)]])
    for q in ([runs(128, 9000)], [runs(64, 6000)]):
        out.append(sk.map_query(q)[0])
    sk.close()
    genomes, queries = _short_inputs()
    p = e.params(16, 500)
    p.windowSize = 300
    sk = Sketch(e, p, genomes)
    for q in queries:
        out.append(sk.map_query([q])[0])
    sk.close()
    c = e.counters()
    e.close()
    return out, c


def _fast_path_against_general(make):
    fast, cf = _map_all(make())
    gen, cg = _map_all(make(ANI_TEST_L2_PATH="general"))
    assert cf["l2FastCandidates"] > 0 and cg["l2FastCandidates"] == 0, (cf, cg)
    assert sum(len(m) for m in fast) >= 40
    for i, (a, b) in enumerate(zip(fast, gen)):
        assert len(a) == len(b) and np.array_equal(a, b), i
    for k in ("l2Steps", "l2WindowEntries", "l2QueryHashes", "l1Candidates"):
        assert cf[k] == cg[k] and cf[k] > 0, (k, cf[k], cg[k])


def test_emu_fast_path_against_general(emu_engine, monkeypatch):
    _fast_path_against_general(lambda **env: _emu(monkeypatch, **env))


@pytest.mark.gpu
def test_gpu_fast_path_against_general(gpu_engine, monkeypatch):
    _fast_path_against_general(lambda **env: _gpu(monkeypatch, **env))
