"""The sketch kernels after their instruction diet (kernels/sketch.hpp, kernels/common.hpp: mul5_add in murmur32_k16, the DPP wave
scans in block_excl_scan and tile_winnow_keys, emission decided by a running maximum, one exchange for the fragment's count and first
window in k_sketch_fused).  Everything is compared bit for bit: reference minimizers with orc.Sketch(...).minimizers(), the fragment
kernel's sketches with orc.fragment_sketch, and the fused all-vs-all pass as parity_cases.case_self does: sketch_records_self ->
Sketch(records=...), its minimizers, the hash count of its fragment set, and the map_cgi_fragset rows against the direct path and
the oracle.  Each case runs on the CPU build of the same sources (tests/emu) and, marked gpu, on the product library.

What the inputs reach:
  packed_lengths   A/C/G/T-only contigs of k-1, k, k+w-2, k+w-1, 2999, 3000, 3001, 3023, 3024, 3072, 6047 and 9100 bases and one of
                   50 000: tile and fragment borders, a fragment's first window, a contig's last tile.  Fragments of 3049 bases put the
                   16 fused tiles of the long contig at all 16 alignments inside a 2-bit word (tile t starts at base 3049 t - 23).
  ties             (ACGT)n and (AT)n are their own reverse complement: hashFwd == hashBwd, the position is skipped.  Homopolymer and
                   (AC)n runs give equal hashes inside one window, where the rightmost position wins.  The runs are 100-200 bases long
                   (every one spans several threads' 12 positions) and lie across the tile borders of both kernels: fused tiles begin at
                   3000 t - (w - 1), the tile kernel's at (3072 - (w - 1)) t.
  windows          12, 13, 24, 25, 47, 48: the prefix / suffix form and its one to four earlier blocks; 11 and 49: span doubling.
  sort forms       3000-base fragments at w = 12 hold more than 256 minimizers (the four-wave sort), 1000-base fragments at w = 48 at most
                   64 (one wave, one key per lane); both asserted from the oracle's sketch sizes.
  other hashes     a contig with N runs and lower case takes the byte path, k = 12 takes murmur32_tail."""
import numpy as np
import pytest

import orc
import parity_cases as pc
from fastani_amd.api import Sketch

K = 16


def _run(length, unit):
    return np.frombuffer((unit * (length // len(unit) + 1))[:length], dtype=np.uint8)


def _with_runs(seed, n, w, frag_len=3000):
    """random bases with low-complexity runs across the borders of the fused tiles and of the tile kernel's tiles"""
    g = pc.rng_genome(seed, n).copy()
    units = [b"ACGT", b"A", b"AC", b"AT", b"T", b"GCGC"]
    stride = 3072 - (w - 1)
    spots = [500, frag_len - (w - 1) - 60, frag_len - 30, stride - 50, 2 * frag_len - (w - 1) - 90, 2 * stride - 100, 3 * frag_len + 7, 3 * stride - 20]
    for i, at in enumerate(spots):
        length = 100 + 20 * (i % 6)
        if 0 <= at and at + length <= n:
            g[at:at + length] = _run(length, units[i % len(units)])
    return g


def _lengths_genomes(w):
    lens = [K - 1, K, K + w - 2, K + w - 1, 2999, 3000, 3001, 3023, 3024, 3072, 6047, 9100]
    return [[pc.rng_genome(100 + i, n) for i, n in enumerate(lens)], [pc.rng_genome(99, 50000)]]


def _check(e, genomes, k, frag_len, w=None):
    """tile kernel, fragment kernel and fused kernel against the oracle; returns the oracle's fragment sketch sizes"""
    p = e.params(k, frag_len)
    if w is not None:
        p.windowSize = w
    w = p.windowSize
    osk = orc.Sketch(genomes, k, w)
    exp_min = osk.minimizers()
    direct = Sketch(e, p, genomes)
    assert np.array_equal(direct.minimizers(), exp_min), (k, frag_len, w)
    exp_fr = []
    for g in genomes:
        for c in g:
            c = orc.upper(c)
            if len(c) >= max(w, k, frag_len):
                exp_fr += [orc.fragment_sketch(c[i * frag_len:(i + 1) * frag_len], k, w) for i in range(len(c) // frag_len)]
    fr = e.query_sketch(p, genomes)
    assert len(fr) == len(exp_fr), (k, frag_len, w)
    for i, (a, b) in enumerate(zip(fr, exp_fr)):
        assert np.array_equal(a, b), (k, frag_len, w, i)
    exp_rows = []
    for qi, g in enumerate(genomes):
        maps, tot = osk.map_genome(g, frag_len)
        exp_rows.append(osk.compute_cgi(maps, tot, qi, frag_len))
    exp_rows = np.concatenate(exp_rows)
    rows0 = direct.map_cgi_batch(genomes, 0)
    assert np.array_equal(rows0, exp_rows), (k, frag_len, w)
    contig_len = np.array([len(c) for g in genomes for c in g], dtype=np.int32)
    gcs = np.cumsum([0] + [len(g) for g in genomes]).astype(np.int32)
    ptr, n, frags = e.sketch_records_self(p, genomes, 0)
    sk = Sketch(e, p, records=(ptr, n, contig_len, gcs))
    assert np.array_equal(sk.minimizers(), exp_min), (k, frag_len, w)
    info = frags.info()
    assert info["fragments"] == len(exp_fr) and info["hashes"] == sum(len(x) for x in exp_fr), (info, k, frag_len, w)
    assert np.array_equal(sk.map_cgi_fragset(frags, 0), exp_rows), (k, frag_len, w)
    if n:
        e.device_free(ptr)
    frags.close()
    sk.close()
    direct.close()
    return [len(x) for x in exp_fr]


def case_packed_lengths(e):
    for frag_len in (3000, 3049):           # 3049 + 24 - 1 = 3072: the largest fragment the fused kernel takes at w = 24
        sizes = _check(e, _lengths_genomes(24), K, frag_len, 24)
        assert len(sizes) >= 20


def case_ties(e):
    genomes = [[_with_runs(7, 13000, 24)], [_with_runs(8, 9500, 24), _run(3100, b"ACGT"), _run(3200, b"A"), _run(3300, b"AC")],
               [pc.mutate(_with_runs(7, 13000, 24), 0.02, 9)]]
    _check(e, genomes, K, 3000, 24)


def case_window(e, w):
    genomes = [[_with_runs(20 + w, 13000, w)], [pc.rng_genome(30 + w, 9100), pc.rng_genome(31 + w, 3000 + w)]]
    _check(e, genomes, K, 3000, w)


def case_sort_forms(e):
    big = _check(e, [[pc.rng_genome(41, 9100)], [pc.rng_genome(42, 6047)]], K, 3000, 12)
    assert max(big) > 256, big              # 2 * 2985 / 13 = 459 expected
    small = _check(e, [[pc.rng_genome(43, 5100)], [pc.rng_genome(44, 3001)]], K, 1000, 48)
    assert max(small) <= 64, small          # 2 * 985 / 49 = 40 expected
    mid = _check(e, [[pc.rng_genome(45, 6047)]], K, 3000, 24)
    assert 64 < min(mid) and max(mid) <= 512, mid


def case_byte_path(e):
    g = pc.rng_genome(51, 12100).copy()
    g[700:760] = ord("N")
    g[2990:3010] = ord("n")
    g[6000:6300] = np.frombuffer(g[6000:6300].tobytes().lower(), dtype=np.uint8)
    g[9050] = ord("R")
    _check(e, [[g, pc.rng_genome(52, 3500, b"ACGTN")], [pc.rng_genome(53, 6047)]], K, 3000)


def case_kmer12(e):
    _check(e, [[_with_runs(61, 9100, 24)], [pc.rng_genome(62, 6047), pc.rng_genome(63, 3024)]], 12, 3000)


WINDOWS = [11, 12, 13, 24, 25, 47, 48, 49]
CASES = [case_packed_lengths, case_ties, case_sort_forms, case_byte_path, case_kmer12]
CASE_IDS = ["packed_lengths", "ties", "sort_forms", "byte_path", "kmer12"]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emu_cases(emu_engine, case):
    case(emu_engine)


@pytest.mark.parametrize("w", WINDOWS)
def test_emu_windows(emu_engine, w):
    case_window(emu_engine, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_cases(gpu_engine, case):
    case(gpu_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS)
def test_gpu_windows(gpu_engine, w):
    case_window(gpu_engine, w)
