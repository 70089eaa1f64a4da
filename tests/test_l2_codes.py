"""k_l2_codes (kernels/l2.hpp) takes its candidates ready-made from LDS (fetch_cands derives them, one thread per candidate), keeps the
current one in scalar registers from pass to pass, and runs a pass in one of two forms: `beyond` (no entry of the first super-window
in it, staged stream: no test per slot) and `general`.  These tests pin every byte it writes through what k_l2_sim makes of it:
every case compares mappings and CGI rows with the CPU oracle, bit for bit; the emulator tests run the same sources on the CPU
(tests/emu), their `gpu` twins the product library.  They hold at the commit before that change as well.

What the inputs cover:
  copies1 .. copies9     one 9-kb query (three fragments) against 1, 2, 3, 4, 5, 7, 9 mutated copies of it as separate reference genomes:
                         a fragment has that many candidates, dealt over the four waves of its workgroup — waves with no candidate,
                         with one (the last item of a wave is also its first), two, three: both hand-overs, pass to pass and candidate
                         to candidate, and a wave's end after either
  batch45, batch81       45 / 81 copies: more than kL2CandBatch = 40 candidates per fragment, one refill of the descriptors in LDS and
                         its two barriers, then two
  short_streams          fragments of 500 bases, window size 300 (the input of test_l2_handover.py): ranges of 5..7 entries, one slot
                         in the last (only) pass, first windows of ONE entry — K = 0, the beyond form from pass 0 on, an all-zero state
  one_entry_windows      the same parameters on the three queries of test_l2_diet.py (mutated at 2, 5, 8 %): more such candidates;
                         the test counts, from the reference minimizers, positions whose super-window holds no second entry
  default                default parameters, ~600 entries per candidate: one window pass, two beyond passes, E = 4, 4 and 2
  window_n_runs          window sizes 19..22 with a 600-base N run per query fragment (class A against first windows of more than 256
                         entries: two window passes, the first window crossing a pass border)
  tandem_repeats         a 21-kb candidate: many passes, a stream beyond the stage window (direct stores, general form throughout),
                         duplicates inside the first window
  low_complexity         near-duplicate entries throughout
  gap_counter_overflow   a field beyond 255 while the first window fills: the overflow mark
each under no knob, ANI_TEST_L2_CHUNK=13 (chunk borders inside a fragment's candidates), ANI_TEST_L2_PATH=classB (80 state dwords: the
second round of the histogram pack) and ANI_TEST_L2_CODE_LIMIT=6000 with ANI_TEST_L2_CHUNK=64.

test_*_fast_path_against_general maps the multi-candidate inputs through the fast path and through ANI_TEST_L2_PATH=general: equal
mappings and equal l2Steps / l2WindowEntries / l2QueryHashes / l1Candidates.  The general kernel does not read the event stream, so
this pins the stream's content independently of the oracle."""
import ctypes
import os

import numpy as np
import pytest

import orc
import parity_cases as pc
from fastani_amd.api import Engine, Sketch

KNOBS = [dict(), dict(ANI_TEST_L2_CHUNK=13), dict(ANI_TEST_L2_PATH="classB"), dict(ANI_TEST_L2_CODE_LIMIT=6000, ANI_TEST_L2_CHUNK=64)]
KNOB_IDS = ["plain", "chunk13", "classB", "codeLimit6000"]
COPIES = (1, 2, 3, 4, 5, 7, 9)


def _copies_inputs(n):
    base = pc.rng_genome(61, 9000)
    return [[pc.mutate(base, 0.02, 100 + i)] for i in range(n)], base


def _map_against_oracle(e, p, genomes, queries, w, frag_len):
    """maps every query through the engine and the oracle, compares mappings and rows bit for bit, returns the oracle's mappings"""
    sk = Sketch(e, p, genomes)
    osk = orc.Sketch(genomes, 16, w)
    out = []
    for qi, q in enumerate(queries):
        maps, tot = sk.map_query(q)
        omaps, otot = osk.map_genome(q, frag_len)
        assert tot == otot and len(maps) == len(omaps), (qi, len(maps), len(omaps))
        assert np.array_equal(maps, omaps), qi
        assert np.array_equal(sk.compute_cgi(maps, tot, qi), osk.compute_cgi(omaps, otot, qi, frag_len)), qi
        out.append(omaps)
    sk.close()
    return out


def _copies(n):
    def case(e):
        """every one of the query's three fragments maps once to each of the n copies: n candidates per fragment"""
        genomes, base = _copies_inputs(n)
        p = e.params(16, 3000)
        omaps = _map_against_oracle(e, p, genomes, [[base]], p.windowSize, 3000)[0]
        for f in range(3):
            refs = omaps["refSeqId"][omaps["querySeqId"] == f]
            assert len(refs) == n and len(np.unique(refs)) == n, (f, len(refs))
        if n > 40:
            assert np.bincount(omaps["querySeqId"]).max() > 40 * ((n - 1) // 40), n
        return True
    case.__name__ = "copies%d" % n
    return case


def _short(ref_seed, queries):
    def case(e):
        ref = pc.rng_genome(ref_seed, 12000)
        genomes = [[ref], [pc.rng_genome(ref_seed + 2, 6000)]]
        p = e.params(16, 500)
        p.windowSize = 300
        # a super-window spans 500 - 299 - 15 = 186 positions: an entry whose successor is at least that far away is a first window of
        # one entry for the candidates that start at it
        wpos = orc.Sketch(genomes, 16, 300).minimizers()
        wpos = wpos["wpos"][wpos["seqId"] == 0]
        assert int((np.diff(wpos) >= 186).sum()) >= 10
        omaps = _map_against_oracle(e, p, genomes, [[pc.mutate(ref, r, sd)] for r, sd in queries], 300, 500)
        assert sum(len(m) for m in omaps) >= 20
        return True
    return case


def _default(e):
    pc.case_synthetic_cluster(e, 30000)
    return True


def _window_n_runs(e):
    """references sketched with windows 19..22 (~270-300 minimizers per 3 kb: first windows beyond one 256-entry pass), queries whose
    fragments each carry a 600-base N run (s <= 255: class A), as in test_l2_handover.py"""
    ref = orc.synth_genome(6, 0, 30000)
    qry = pc.mutate(ref, 0.03, 11)
    for f in range(len(qry) // 3000):
        qry[f * 3000 + 1200:f * 3000 + 1800] = ord("N")
    genomes = [[ref], [orc.synth_genome(6, 2, 9000)]]
    for w in (19, 20, 21, 22):
        p = e.params(16, 3000)
        p.windowSize = w
        fr = e.query_sketch(p, [[qry]])
        assert len(fr) == 10 and max(len(x) for x in fr) <= 255, [len(x) for x in fr]
        omaps = _map_against_oracle(e, p, genomes, [[qry]], w, 3000)[0]
        assert len(omaps) >= 8, (w, len(omaps))
    return True


def _no_bar(case):
    def run(e):
        case(e)
        return False                              # candidates beyond the fast path's limits or overflowing counters are part of the input
    return run


CASES = [_copies(n) for n in COPIES] + [_copies(45), _copies(81), _short(41, [(0.02, 42)]), _short(51, [(0.02, 52), (0.05, 54), (0.08, 54)]),
                                         _default, _window_n_runs, pc.case_tandem_repeats, pc.case_low_complexity,
                                         _no_bar(pc.case_gap_counter_overflow)]
CASE_IDS = ["copies%d" % n for n in COPIES] + ["batch45", "batch81", "short_streams", "one_entry_windows", "default", "window_n_runs",
                                               "tandem_repeats", "low_complexity", "gap_counter_overflow"]


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
    no_overflow = case(e) is not False
    c = e.counters()
    e.close()
    assert c["l2FastCandidates"] > 0, c
    if no_overflow:
        assert c["l2SlowCandidates"] == 0, c


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emu_cases(emu_engine, monkeypatch, case, knobs):
    _run_case(_emu(monkeypatch, **knobs), case)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_cases(gpu_engine, monkeypatch, case, knobs):
    _run_case(_gpu(monkeypatch, **knobs), case)


def _map_copies(e):
    """mappings and L2 counters of the multi-candidate inputs"""
    out = []
    e.reset_counters()
    for n in COPIES + (45, 81):
        genomes, base = _copies_inputs(n)
        sk = Sketch(e, e.params(16, 3000), genomes)
        out.append(sk.map_query([base])[0])
        sk.close()
    c = e.counters()
    e.close()
    return out, c


def _fast_path_against_general(make):
    fast, cf = _map_copies(make())
    gen, cg = _map_copies(make(ANI_TEST_L2_PATH="general"))
    assert cf["l2FastCandidates"] > 0 and cf["l2SlowCandidates"] == 0 and cg["l2FastCandidates"] == 0, (cf, cg)
    for i, (a, b) in enumerate(zip(fast, gen)):
        assert len(a) == len(b) == 3 * (COPIES + (45, 81))[i] and np.array_equal(a, b), i
    for k in ("l2Steps", "l2WindowEntries", "l2QueryHashes", "l1Candidates"):
        assert cf[k] == cg[k] and cf[k] > 0, (k, cf[k], cg[k])


def test_emu_fast_path_against_general(emu_engine, monkeypatch):
    _fast_path_against_general(lambda **env: _emu(monkeypatch, **env))


@pytest.mark.gpu
def test_gpu_fast_path_against_general(gpu_engine, monkeypatch):
    _fast_path_against_general(lambda **env: _gpu(monkeypatch, **env))
