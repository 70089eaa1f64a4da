"""Whole-genome sketch ANI (ani_sketch_signatures, ani_signature_pairs, fastANI --sketchANI / --tree --treeFill sketch) against a numpy
statement of its integer semantics (include/ani_abi.h, rules 1 - 3).
CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases
import orc
import fastani_amd
from fastani_amd.api import SIGPAIR_DT, AniError
from test_cluster import make_rows, read_matrix
from test_emu_parity import _emu_engine_with
from test_gpu_parity import _engine_with
from test_tree import parse_newick
from test_tree_nj import parse_unrooted, splits_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the semantics, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def signatures_expected(minimizers, contigs_per_genome, size):
    """rule 1 from the position-ordered minimizer records and the contig -> genome table"""
    contig_genome = np.repeat(np.arange(len(contigs_per_genome)), contigs_per_genome)
    n = len(contigs_per_genome)
    sig = np.zeros((n, size), dtype=np.uint32)
    length = np.zeros(n, dtype=np.int32)
    genome = contig_genome[minimizers["seqId"]] if len(minimizers) else np.zeros(0, dtype=np.int64)
    for g in range(n):
        h = np.unique(minimizers["hash"][genome == g])[:size]
        sig[g, :len(h)] = h
        length[g] = len(h)
    return sig, length


def pair_expected(x, y, size):
    """rule 2 for two ascending distinct arrays -> (shared, size)"""
    u = np.union1d(x, y)[:size]
    return int(np.isin(u, x, assume_unique=True).astype(np.int64) @ np.isin(u, y, assume_unique=True).astype(np.int64)), len(u)


def identity_expected(shared, size, k):
    """rule 3: one double expression from the exact integers, rounded once to float"""
    if shared == 0:
        return np.float32(0.0)
    v = 100.0 * (1.0 + np.log(2.0 * np.float64(shared) / np.float64(size + shared)) / np.float64(k))
    return np.float32(min(max(v, 0.0), 100.0))


def pairs_expected(sig, length, k, min_shared):
    n, size = sig.shape
    out = []
    for a in range(n):
        for b in range(a + 1, n):
            sh, sz = pair_expected(sig[a, :length[a]], sig[b, :length[b]], size)
            if sh >= min_shared:
                out.append((a, b, sh, sz, identity_expected(sh, sz, k)))
    return np.array(out, dtype=SIGPAIR_DT)


def ulp_apart(x, y):
    """distance in float32 steps between non-negative floats"""
    return np.abs(x.astype(np.float32).view(np.int32).astype(np.int64) - y.astype(np.float32).view(np.int32).astype(np.int64))


def check_pairs(engine, sig, length, k=16, min_shared=1):
    got = engine.signature_pairs(sig, length, k, min_shared)
    want = pairs_expected(sig, length, k, min_shared)
    assert got.dtype == SIGPAIR_DT
    assert len(got) == len(want), (len(got), len(want))
    for f in ("a", "b", "shared", "size"):
        assert np.array_equal(got[f], want[f]), f
    # One correctly ordered double expression rounded once: a libm log that differs in its last double bit moves the float by at most
    # one step, and only at a rounding boundary.
    assert (ulp_apart(got["identity"], want["identity"]) <= 1).all()
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# signatures against the pinned minimizers
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 7, 1000, 4096)


def signature_inputs():
    c = golden_cases.cases()
    short = golden_cases._rng(12, 2500)                           # fewer than 1000 distinct hashes
    return {"evolved": (c["evolved"][0], 16), "onehash": (c["onehash"][0], 16), "repeats": (c["repeats"][0] + [[short]], 16),
            "messy": (c["messy"][0] + [[np.frombuffer(b"ACGTA", dtype=np.uint8)]], 16),     # an N-ridden multi-contig genome, a 10-base and a 5-base one: empty
            "manycontigs": (c["manycontigs"][0], 16), "k12": (c["k12"][0], 12)}


def check_signatures(engine, names=None, sizes=SIZES):
    seen_short = seen_empty = False
    for name, (genomes, k) in signature_inputs().items():
        if names is not None and name not in names:
            continue
        p = engine.params(k, 3000)
        sk = fastani_amd.Sketch(engine, p, genomes)
        mins = sk.minimizers()
        for size in sizes:
            sig, length = sk.signatures(size)
            want_sig, want_len = signatures_expected(mins, [len(g) for g in genomes], size)
            assert sig.dtype == np.uint32 and sig.shape == (len(genomes), size) and length.dtype == np.int32
            assert np.array_equal(length, want_len), (name, size, length, want_len)
            assert np.array_equal(sig, want_sig), (name, size)
            seen_short |= bool(((want_len > 0) & (want_len < size)).any()) and size == 1000
            seen_empty |= bool((want_len == 0).any())
        sk.close()
    if names is None:
        assert seen_short and seen_empty


def test_signatures_cpu_build(emu_engine):
    check_signatures(emu_engine)


def test_signatures_chunked_cpu_build(monkeypatch):
    e = _emu_engine_with(monkeypatch, ANI_MAX_INDEX_MINIMIZERS=4000)
    sk = fastani_amd.Sketch(e, e.params(16, 3000), signature_inputs()["evolved"][0])
    assert len(sk.chunks()) >= 3
    sk.close()
    check_signatures(e, ("evolved", "messy", "repeats"))


def test_signatures_streamed_cpu_build(monkeypatch):
    e = _emu_engine_with(monkeypatch, ANI_MAX_INDEX_MINIMIZERS=4000, ANI_MAX_RESIDENT_CHUNKS=1)
    check_signatures(e, ("evolved", "messy", "onehash"))


def sketch_file_range(engine, tmp):
    genomes, k = signature_inputs()["evolved"]
    p = engine.params(k, 3000)
    sk = fastani_amd.Sketch(engine, p, genomes)
    path = os.path.join(tmp, "fam.anisk")
    sk.save(path, ["g%d" % i for i in range(len(genomes))])
    full = {size: sk.signatures(size) for size in (7, 1000)}
    sk.close()
    for g0, g1 in ((0, -1), (1, 4), (2, 3), (5, 6)):
        part = fastani_amd.Sketch(engine, p, file=path, genome_range=(g0, g1))
        hi = len(genomes) if g1 < 0 else g1
        want_sig, want_len = signatures_expected(part.minimizers(), [len(g) for g in genomes[g0:hi]], 1000)
        for size in (7, 1000):
            sig, length = part.signatures(size)
            assert np.array_equal(sig, full[size][0][g0:hi]) and np.array_equal(length, full[size][1][g0:hi]), (g0, g1, size)
        assert np.array_equal(part.signatures(1000)[0], want_sig) and np.array_equal(part.signatures(1000)[1], want_len)
        part.close()


def test_signatures_sketch_file_cpu_build(emu_engine, tmp_path):
    sketch_file_range(emu_engine, str(tmp_path))


def test_signatures_sketch_file_streamed_cpu_build(monkeypatch, tmp_path):
    sketch_file_range(_emu_engine_with(monkeypatch, ANI_MAX_INDEX_MINIMIZERS=4000, ANI_MAX_RESIDENT_CHUNKS=1), str(tmp_path))


@pytest.mark.gpu
def test_signatures_gpu(gpu_engine, tmp_path):
    check_signatures(gpu_engine)
    sketch_file_range(gpu_engine, str(tmp_path))


@pytest.mark.gpu
def test_signatures_chunked_gpu(monkeypatch):
    check_signatures(_engine_with(monkeypatch, ANI_MAX_INDEX_MINIMIZERS=4000), ("evolved", "messy", "repeats"))


@pytest.mark.gpu
def test_signatures_streamed_gpu(monkeypatch, tmp_path):
    e = _engine_with(monkeypatch, ANI_MAX_INDEX_MINIMIZERS=4000, ANI_MAX_RESIDENT_CHUNKS=1)
    check_signatures(e, ("evolved", "messy", "onehash"))
    sketch_file_range(e, str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------------------------
# pairs against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def make_signatures(sets, size):
    """ascending distinct arrays -> (sig, length) at `size` (each set cut to its `size` smallest)"""
    sig = np.zeros((len(sets), size), dtype=np.uint32)
    length = np.zeros(len(sets), dtype=np.int32)
    for i, s in enumerate(sets):
        s = np.unique(np.asarray(s, dtype=np.uint32))[:size]
        sig[i, :len(s)] = s
        length[i] = len(s)
    return sig, length


def random_sets(rng, n, size, universe, full=0.6):
    """n sets over `universe` values: related ones (families share a base set), lengths 0 and below `size` mixed with full ones"""
    sets = []
    base = None
    for i in range(n):
        if base is None or rng.random() < 0.2:
            base = rng.choice(universe, size=min(universe, 2 * size), replace=False)
        keep = base[rng.random(len(base)) < rng.uniform(0.3, 1.0)]
        extra = rng.integers(0, universe, int(rng.integers(0, size)))
        s = np.concatenate([keep, extra])
        u = rng.random()
        if u > full:
            s = s[:int(rng.integers(0, size))] if u < 0.95 else s[:0]
        sets.append(s.astype(np.uint32) * np.uint32(2 ** 32 // universe - 1) + np.uint32(i % 2 if u < 0.1 else 0))
    return sets


def pair_cases(engine, big):
    rng = np.random.default_rng(5)
    # n of 0, 1, 2
    for n in (0, 1):
        got = engine.signature_pairs(np.zeros((n, 9), dtype=np.uint32), np.zeros(n, dtype=np.int32), 16, 0)
        assert got.dtype == SIGPAIR_DT and len(got) == 0
    a = np.arange(10, 30)
    # identical, disjoint, nested, empty: hand-checked values
    sig, length = make_signatures([a, a, a + 100, a[:5], []], 8)
    got = check_pairs(engine, sig, length, 16, 0)
    assert len(got) == 10
    by = {(int(r["a"]), int(r["b"])): (int(r["shared"]), int(r["size"])) for r in got}
    assert by[(0, 1)] == (8, 8) and by[(0, 2)] == (0, 8) and by[(0, 3)] == (5, 8) and by[(0, 4)] == (0, 8) and by[(3, 4)] == (0, 5)
    assert got["identity"][0] == 100.0 and got["identity"][1] == 0.0
    sig, length = make_signatures([[], []], 3)
    assert engine.signature_pairs(sig, length, 16, 0).tolist() == [(0, 1, 0, 0, 0.0)]
    assert len(engine.signature_pairs(sig, length, 16, 1)) == 0
    # the largest hash value, a union shorter than the size, one value
    sig, length = make_signatures([[0xffffffff], [0xffffffff, 5], [0xfffffffe, 0xffffffff]], 4)
    check_pairs(engine, sig, length, 16, 0)
    # random, ragged on both tile axes (tile edges 16, 8 and 4 by size), every size class
    for n, size, universe in ((2, 1, 50), (17, 5, 40), (33, 64, 300), (50, 257, 3000), (21, 1000, 6000), (19, 1025, 9000), (11, 2049, 20000), (9, 4096, 30000)) + \
            (((300, 37, 400), (130, 1000, 7000)) if big else ((70, 37, 400), (210, 24, 300))):
        sig, length = make_signatures(random_sets(rng, n, size, universe), size)
        for ms in (0, 1, max(2, size // 8), size + 1):
            check_pairs(engine, sig, length, int(rng.integers(1, 17)), ms)
    # every tile edge with identical rows: shared = size on and off the diagonal
    full = np.sort(rng.choice(1 << 32, size=4096, replace=False)).astype(np.uint32)
    for size in (256, 1024, 2048, 4096):
        n = 9
        got = engine.signature_pairs(np.tile(full[:size], (n, 1)), np.full(n, size, dtype=np.int32), 16)
        assert len(got) == n * (n - 1) // 2 and (got["shared"] == size).all() and (got["size"] == size).all() and (got["identity"] == 100.0).all()


def test_restatement_by_hand():
    # U = 1 2 3 4 5 6 ..., size 4: the first four of U are 1 2 3 4, of which 2 and 4 are in both
    assert pair_expected(np.array([1, 2, 4, 6, 8]), np.array([2, 3, 4, 5, 6]), 4) == (2, 4)
    assert pair_expected(np.array([1, 2]), np.array([2, 3]), 10) == (1, 3)
    assert identity_expected(10, 10, 16) == 100.0 and identity_expected(0, 10, 16) == 0.0
    assert abs(float(identity_expected(5, 1000, 16)) - 100 * (1 + np.log(10 / 1005) / 16)) < 1e-5


def test_pairs_cpu_build(emu_engine):
    pair_cases(emu_engine, False)


@pytest.mark.gpu
def test_pairs_gpu(gpu_engine):
    pair_cases(gpu_engine, True)


def all_pairs_vectorised(sig, length, universe_step):
    """every pair's (shared, size) by another route than pair_expected: per genome a, the rank of every value of the later rows in the
    union with row a comes from count tables over the value universe (values are multiples of universe_step)"""
    n, size = sig.shape
    idx = (sig // universe_step).astype(np.int64)
    m = int(idx.max()) + 2
    member = np.zeros((n, m), dtype=bool)
    for g in range(n):
        member[g, idx[g, :length[g]]] = True
    below = np.cumsum(member, axis=1, dtype=np.int32) - member            # values of g strictly below v
    valid = np.arange(size)[None, :] < length[:, None]
    shared = np.zeros((n, n), dtype=np.int32)
    usize = np.zeros((n, n), dtype=np.int32)

    def row(a):
        if a + 1 >= n:
            return
        bi = idx[a + 1:]
        isin = member[a][bi] & valid[a + 1:]
        # values of the union at or below b's j-th value: j + 1 of b, those of a below it or equal, less the shared ones counted twice
        rank = np.arange(1, size + 1)[None, :] + below[a][bi] + isin - np.cumsum(isin, axis=1)
        shared[a, a + 1:] = (isin & (rank <= size)).sum(axis=1)
        usize[a, a + 1:] = np.minimum(size, length[a] + length[a + 1:] - isin.sum(axis=1))

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(row, range(n)))
    return shared, usize


def test_vectorised_restatement_agrees():
    rng = np.random.default_rng(9)
    step = 1000
    sets = [np.sort(rng.choice(400, size=int(rng.integers(0, 120)), replace=False)) * step for _ in range(25)]
    sig, length = make_signatures(sets, 64)
    shared, usize = all_pairs_vectorised(sig, length, step)
    for a in range(25):
        for b in range(a + 1, 25):
            assert (shared[a, b], usize[a, b]) == pair_expected(sig[a, :length[a]], sig[b, :length[b]], 64), (a, b)


@pytest.mark.gpu
def test_pairs_large_gpu(gpu_engine):
    """3000 genomes at s = 1000: a sample of pairs against the restatement, and the row count and a checksum over all 4.5 million pairs
    against the vectorised host pass"""
    rng = np.random.default_rng(21)
    n, size, universe, step = 3000, 1000, 6000, 700000
    sets = []
    for g in range(n):
        density = rng.uniform(0.05, 0.7)
        s = np.flatnonzero(rng.random(universe) < density)
        sets.append(s.astype(np.uint32) * np.uint32(step))
    sig, length = make_signatures(sets, size)
    assert (length < size).any() and (length == size).sum() > n // 2
    shared, usize = all_pairs_vectorised(sig, length, step)
    for min_shared in (1, 300):
        got = gpu_engine.signature_pairs(sig, length, 16, min_shared)
        iu = np.triu_indices(n, 1)
        keep = shared[iu] >= min_shared
        assert len(got) == int(keep.sum())
        assert np.array_equal(got["a"], iu[0][keep]) and np.array_equal(got["b"], iu[1][keep])
        assert np.array_equal(got["shared"], shared[iu][keep]) and np.array_equal(got["size"], usize[iu][keep])
        weight = (got["a"].astype(np.int64) * 7919 + got["b"].astype(np.int64) * 104729) % 1000003
        want_w = (iu[0][keep].astype(np.int64) * 7919 + iu[1][keep].astype(np.int64) * 104729) % 1000003
        assert int((weight * (got["shared"].astype(np.int64) * 4099 + got["size"])).sum()) == int((want_w * (shared[iu][keep].astype(np.int64) * 4099 + usize[iu][keep])).sum())
        pick = rng.choice(len(got), size=300, replace=False)
        for r in got[pick]:
            a, b = int(r["a"]), int(r["b"])
            assert (int(r["shared"]), int(r["size"])) == pair_expected(sig[a, :length[a]], sig[b, :length[b]], size)
            assert ulp_apart(np.array([r["identity"]]), np.array([identity_expected(int(r["shared"]), int(r["size"]), 16)]))[0] <= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# real-shaped data: an ancestor and descendants mutated at growing rates
# ---------------------------------------------------------------------------------------------------------------------------------
RATES = (0.02, 0.08, 0.15, 0.22, 0.32, 0.34, 0.36)


def descendants(n=56000, seed=49):
    """(seed and length are chosen so that no fragment of the last descendant maps to the ancestor, or back, by luck: at these rates
    two or three of its eighteen fragments usually still do)"""
    anc = golden_cases._rng(seed, n)
    seeds = [100 * seed + 10 + i for i in range(4)] + [100 * seed + 3 + i for i in range(3)]
    return [[anc]] + [[golden_cases.evolve(anc, sd, sub=r, indel=0.002, inversions=1, duplications=0, translocations=0)] for sd, r in zip(seeds, RATES)]


def evolved_behaviour(engine):
    """The estimate to the ancestor falls strictly with the substitution rate.  A draw replaces a base by itself one time in four, so
    the rates are 1.5 to 27 % of differing bases; at the last one a 16-mer survives with probability 0.73^16 = 0.0065, which is a
    Jaccard index of 0.003: about 13 shared values at s = 4096, while the mapping has no fragment left that far below 80 % identity."""
    genomes = descendants()
    p = engine.params(16, 3000)
    sk = fastani_amd.Sketch(engine, p, genomes)
    sig, length = sk.signatures(4096)
    assert (length == 4096).all()
    pairs = engine.signature_pairs(sig, length, 16, 0)
    to_anc = pairs[pairs["a"] == 0]
    assert to_anc["b"].tolist() == list(range(1, len(RATES) + 1))
    est = to_anc["identity"].astype(np.float64)
    assert (np.diff(est) < 0).all(), est
    assert est[0] > 95 and est[-1] < 85
    rows = sk.map_cgi_batch(genomes, 0)
    with_anc = {int(r["qryGenomeId"]) + int(r["refGenomeId"]) for r in rows if min(r["qryGenomeId"], r["refGenomeId"]) == 0 and r["qryGenomeId"] != r["refGenomeId"]}
    assert 1 in with_anc                                                      # the close descendant is mapped
    silent = [g for g in range(1, len(RATES) + 1) if g not in with_anc]
    assert silent and all(to_anc["shared"][g - 1] >= 8 for g in silent), (silent, to_anc["shared"])
    sk.close()


def test_evolved_behaviour_cpu_build(emu_engine):
    evolved_behaviour(emu_engine)


@pytest.mark.gpu
def test_evolved_behaviour_gpu(gpu_engine):
    evolved_behaviour(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    lib, h = engine.lib, engine.h

    def call(sig_p, len_p, n, size, k, ms, rows=True, cnt=True):
        p, m = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib.ani_signature_pairs(h, sig_p, len_p, n, size, k, ms, ctypes.byref(p) if rows else None, ctypes.byref(m) if cnt else None)
        if rc == 0:
            lib.ani_free(p)
        return rc

    s, l = sig.ctypes.data, length.ctypes.data
    assert call(s, l, 3, 3, 16, 1) == 0
    for size in (0, -1, 4097):
        assert call(s, l, 3, size, 16, 1) == -1, size
    for k in (0, -3, 17):
        assert call(s, l, 3, 3, k, 1) == -1, k
    assert call(s, l, 3, 3, 16, -1) == -1
    assert call(s, l, -1, 3, 16, 1) == -1
    assert call(None, l, 3, 3, 16, 1) == -1 and call(s, None, 3, 3, 16, 1) == -1
    assert call(s, l, 3, 3, 16, 1, rows=False) == -1 and call(s, l, 3, 3, 16, 1, cnt=False) == -1
    assert lib.ani_signature_pairs(None, s, l, 3, 3, 16, 1, ctypes.byref(ctypes.c_void_p()), ctypes.byref(ctypes.c_size_t())) == -1
    assert call(s, l, 65537, 3, 16, 1) == -4                      # the limit, before anything is read or allocated
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.signature_pairs(sig, np.array(bad_len, dtype=np.int32), 16)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.signature_pairs(x, length, 16)
        assert ex.value.code == -1, bad_row
    x = sig.copy()
    x[2] = [9, 9, 1]                                              # beyond the length: not looked at
    assert len(engine.signature_pairs(x, length, 16, 0)) == 3
    # a lone row is checked too
    with pytest.raises(AniError) as ex:
        engine.signature_pairs(np.array([[3, 2, 1]], dtype=np.uint32), np.array([3], dtype=np.int32), 16)
    assert ex.value.code == -1
    assert len(engine.signature_pairs(np.array([[3, 2, 1]], dtype=np.uint32), np.array([1], dtype=np.int32), 16)) == 0
    # the sketch side
    p = engine.params(16, 3000)
    sk = fastani_amd.Sketch(engine, p, [[orc.synth_genome(3, 0, 9000)]])
    for size in (0, -5, 4097):
        with pytest.raises(AniError) as ex:
            sk.signatures(size)
        assert ex.value.code == -1, size
    buf, ln = np.zeros(8, dtype=np.uint32), np.zeros(1, dtype=np.int32)
    assert lib.ani_sketch_signatures(None, 8, buf.ctypes.data, ln.ctypes.data) == -1
    assert lib.ani_sketch_signatures(sk.h, 8, None, ln.ctypes.data) == -1 and lib.ani_sketch_signatures(sk.h, 8, buf.ctypes.data, None) == -1
    assert lib.ani_sketch_signatures(sk.h, 8, buf.ctypes.data, ln.ctypes.data) == 0 and ln[0] == 8 and (np.diff(buf.astype(np.int64)) > 0).all()
    sk.close()
    # a set without genomes
    empty = fastani_amd.Sketch(engine, p, [])
    sig0, len0 = empty.signatures(5)
    assert sig0.shape == (0, 5) and len0.shape == (0,)
    empty.close()


def test_errors_cpu_build(emu_engine):
    argument_errors(emu_engine)


@pytest.mark.gpu
def test_errors_gpu(gpu_engine):
    argument_errors(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
CLI_MODES = [("sliced", {"ANI_SLICE_BYTES": "40000"}, []),
             ("chunked", {"ANI_SLICE_BYTES": "40000", "ANI_MAX_INDEX_MINIMIZERS": "7000"}, []),
             ("streamed", {"ANI_SLICE_BYTES": "40000", "ANI_MAX_INDEX_MINIMIZERS": "7000", "ANI_MAX_RESIDENT_CHUNKS": "1"}, []),
             ("devices", {"ANI_SLICE_BYTES": "40000"}, ["--devices", "0,0"]),
             ("gpus1", {}, ["--gpus", "1"]),
             ("sanity", {}, ["-s"]),
             ("sanity3", {}, ["-s", "-t", "3"])]


def two_genera(tmp, n_len):
    """Two genera from one ancestor: three close relatives of the ancestor and three of a descendant at 38 % substitutions.  The mapping
    has nothing to say between the genera; their sketches still share a few values.  One file name needs quoting."""
    anc = golden_cases._rng(77, n_len)
    far = golden_cases.evolve(anc, 78, sub=0.38, indel=0.002, inversions=1, duplications=0, translocations=0)
    seqs = [golden_cases._mutate(anc, r, 80 + i) for i, r in enumerate((0.0, 0.02, 0.05))] + [golden_cases._mutate(far, r, 90 + i) for i, r in enumerate((0.0, 0.03, 0.06))]
    paths = []
    for i, s in enumerate(seqs):
        p = os.path.join(tmp, "g %d.fa" % i if i == 4 else "g%d.fa" % i)
        orc.write_fasta(p, [s], names=["c%d" % i])
        paths.append(p)
    lst = os.path.join(tmp, "l.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst, paths, [[s] for s in seqs]


def linkage_clades(z, names):
    """scipy linkage rows -> {clade: branch length above it}, as test_tree.tree_from_matrix"""
    n = len(names)
    clade = [frozenset([x]) for x in names]
    h = [0.0] * n
    lengths = {}
    for x, y, height, _ in z.tolist():
        for c in (int(x), int(y)):
            lengths[clade[c]] = (float(height) - h[c]) / 2
        clade.append(clade[int(x)] | clade[int(y)])
        h.append(float(height))
    return lengths


def run(binary, args, env=None):
    r = subprocess.run([binary] + args, capture_output=True, env=dict(os.environ, **(env or {})))
    return r


def run_cli(binary, engine, tmp, n_len):
    size, min_ani = 2000, 60.0
    lst, paths, genomes = two_genera(tmp, n_len)
    n = len(paths)
    common = ["--ql", lst, "--rl", lst, "--matrix", "--cluster", "95"]
    base = os.path.join(tmp, "base.out")
    r = run(binary, common + ["--tree", "-o", base])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert not os.path.exists(base + ".sketch")
    out = os.path.join(tmp, "fill.out")
    r = run(binary, common + ["--tree", "--treeFill", "sketch", "--sketchANI", "--sketchSize", str(size), "--sketchMinANI", str(min_ani), "-o", out],
            {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"signatures collected" in r.stderr and b"sketch pairs compared" in r.stderr
    for ext in ("", ".matrix", ".clusters"):
        assert open(out + ext, "rb").read() == open(base + ext, "rb").read(), ext
    # the API on the same genomes
    sk = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes)
    sig, length = sk.signatures(size)
    sk.close()
    pairs = engine.signature_pairs(sig, length, 16, 1)
    want = "".join("%s\t%s\t%s\t%d/%d\n" % (paths[r["a"]], paths[r["b"]], "%g" % r["identity"], r["shared"], r["size"]) for r in pairs if r["identity"] >= min_ani)
    text = open(out + ".sketch").read()
    assert text == want
    assert len(text.splitlines()) >= 9                                                  # both genera inside, and something across
    # the tree: rows of the printed .matrix + the fill rows, through the API
    names, cells = read_matrix(base + ".matrix")
    assert names == paths
    rows = [(j, i, np.float32(cells[(j, i)])) for j, i in sorted(cells)]
    have = {(min(i, j), max(i, j)) for j, i in cells}
    fill = [(int(r["a"]), int(r["b"]), r["identity"]) for r in pairs if (int(r["a"]), int(r["b"])) not in have and r["identity"] > 0]
    across = [(a, b) for a in range(3) for b in range(3, 6)]
    assert not any(x in have for x in across), "the genera were meant to be out of the mapping's reach"
    assert {(a, b) for a, b, _ in fill} <= set(across) and len(fill) >= 3
    z0 = engine.tree_average(make_rows(rows), n, 0.0)
    z1 = engine.tree_average(make_rows(rows + fill), n, 0.0)
    assert z0[-1, 2] == 1.0                                                             # without the fill the genera meet at distance 1
    est = {(a, b): float(w) for a, b, w in fill}
    top = np.mean([1.0 - est.get(x, 0.0) / 100.0 for x in across])                      # average linkage of the nine pairs across
    assert abs(z1[-1, 2] - top) < 1e-6 and z1[-1, 2] < 0.9
    for path, z in ((base, z0), (out, z1)):
        got, root = parse_newick(open(path + ".newick").read())
        want_l = linkage_clades(z, names)
        assert root == frozenset(names) and set(got) == set(want_l)
        for c in want_l:
            assert abs(got[c] - want_l[c]) <= 1e-6, (sorted(c), got[c], want_l[c])
    # two genomes, one of each genus: no cell, so the root sits at distance 1 without the fill and at 1 - estimate / 100 with it
    two = os.path.join(tmp, "two.txt")
    open(two, "w").write(paths[0] + "\n" + paths[3] + "\n")
    e03 = [float(r["identity"]) for r in pairs if (r["a"], r["b"]) == (0, 3)]
    assert len(e03) == 1 and 50 < e03[0] < 90
    for extra, height in (([], 1.0), (["--treeFill", "sketch", "--sketchSize", str(size)], 1.0 - e03[0] / 100.0)):
        o = os.path.join(tmp, "two%d.out" % len(extra))
        r = run(binary, ["--ql", two, "--rl", two, "--matrix", "--tree"] + extra + ["-o", o])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert open(o + ".matrix").read().splitlines()[2].split("\t")[1] == "NA"
        got, _ = parse_newick(open(o + ".newick").read())
        assert abs(got[frozenset([paths[0]])] - height / 2) < 1e-6 and abs(got[frozenset([paths[3]])] - height / 2) < 1e-6, (got, height)
    # neighbour joining with the fill
    nj_base, nj_out = os.path.join(tmp, "njb.out"), os.path.join(tmp, "nj.out")
    assert run(binary, common + ["--tree", "--treeMethod", "nj", "-o", nj_base]).returncode == 0
    r = run(binary, common + ["--tree", "--treeMethod", "nj", "--treeFill", "sketch", "--sketchSize", str(size), "-o", nj_out])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert not os.path.exists(nj_out + ".sketch")
    for ext in ("", ".matrix", ".clusters"):
        assert open(nj_out + ext, "rb").read() == open(base + ext, "rb").read(), ext
    assert open(nj_out + ".newick").read() != open(nj_base + ".newick").read()
    children, branch = engine.tree_nj(make_rows(rows + fill), n, 0.0)
    want_s = {frozenset(frozenset(names[i] for i in side) for side in k): v for k, v in splits_of(children, branch, n).items()}
    got_l, top3 = parse_unrooted(open(nj_out + ".newick").read())
    everyone = frozenset(names)
    got_s = {frozenset([c, everyone - c]): v for c, v in got_l.items()}
    assert set(got_s) == set(want_s)
    for k in want_s:
        assert abs(got_s[k] - want_s[k]) <= 1e-6, (got_s[k], want_s[k])
    # --sketchANI alone, default size and threshold: nothing else changes, no tree
    alone = os.path.join(tmp, "alone.out")
    r = run(binary, ["--ql", lst, "--rl", lst, "--sketchANI", "-o", alone])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(alone, "rb").read() == open(base, "rb").read() and not os.path.exists(alone + ".newick") and not os.path.exists(alone + ".matrix")
    sig1, len1 = fastani_amd.Sketch(engine, engine.params(16, 3000), genomes).signatures(1000)
    p1 = engine.signature_pairs(sig1, len1, 16, 1)
    assert open(alone + ".sketch").read() == "".join("%s\t%s\t%s\t%d/%d\n" % (paths[r["a"]], paths[r["b"]], "%g" % r["identity"], r["shared"], r["size"])
                                                     for r in p1 if r["identity"] >= 70.0)
    # the same files through the other paths of the command line
    fill_args = ["--tree", "--treeFill", "sketch", "--sketchANI", "--sketchSize", str(size), "--sketchMinANI", str(min_ani)]
    for name, env, args in CLI_MODES:
        o = os.path.join(tmp, "m_%s.out" % name)
        r = run(binary, common + args + fill_args + ["-o", o], env)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        for ext in (".sketch", ".newick", ".matrix", ".clusters"):
            assert open(o + ext, "rb").read() == open(out + ext, "rb").read(), (name, ext)
    # --visualize (the per-query mapping path, two reference splits): .visual and the rest byte for byte with and without the options
    vis0, vis1 = os.path.join(tmp, "vis0.out"), os.path.join(tmp, "vis1.out")
    r = run(binary, common + ["-t", "2", "--visualize", "--tree", "-o", vis0])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    r = run(binary, common + ["-t", "2", "--visualize"] + fill_args + ["-o", vis1])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert os.path.getsize(vis0 + ".visual") > 0 and not os.path.exists(vis0 + ".sketch")
    for ext in ("", ".matrix", ".clusters", ".visual"):
        assert open(vis1 + ext, "rb").read() == open(vis0 + ext, "rb").read(), ext
    assert open(vis0 + ".matrix", "rb").read() == open(base + ".matrix", "rb").read()
    assert open(vis0 + ".newick", "rb").read() == open(base + ".newick", "rb").read()
    for ext in (".sketch", ".newick"):
        assert open(vis1 + ext, "rb").read() == open(out + ext, "rb").read(), ext
    # a reference sketch file, whole and in blocks of genomes
    skf = os.path.join(tmp, "refs.anisk")
    assert run(binary, common + ["--saveSketch", skf, "-o", os.path.join(tmp, "save.out")]).returncode == 0
    for name, env, args in (("file", {}, []), ("blocks", {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, []),
                            ("blocks2", {"ANI_CLI_REF_BLOCK_BYTES": "30000", "ANI_MAX_INDEX_MINIMIZERS": "5000", "ANI_MAX_RESIDENT_CHUNKS": "1"}, ["--devices", "0,0"])):
        o = os.path.join(tmp, "f_%s.out" % name)
        r = run(binary, ["--ql", lst, "--refSketch", skf, "--matrix", "--cluster", "95"] + args + fill_args + ["-o", o], env)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        for ext in (".sketch", ".newick", ".matrix", ".clusters"):
            assert open(o + ext, "rb").read() == open(out + ext, "rb").read(), (name, ext)
    # refusals
    bad = os.path.join(tmp, "bad.out")
    for args, msg in ((["--treeFill", "sketch"], b"--treeFill needs --tree"), (["--tree", "--treeFill", "mash"], b"--treeFill takes none or sketch"),
                      (["--sketchSize", "500"], b"--sketchSize needs --sketchANI or --treeFill sketch"), (["--sketchMinANI", "80"], b"--sketchMinANI needs --sketchANI"),
                      (["--sketchANI", "--sketchSize", "0"], b"--sketchSize takes a size from 1 to 4096"),
                      (["--sketchANI", "--sketchSize", "4097"], b"--sketchSize takes a size from 1 to 4096"),
                      (["--sketchANI", "--sketchMinANI", "101"], b"--sketchMinANI takes an ANI in [0, 100]"),
                      (["--sketchANI", "--sketchMinANI", "-1"], b"--sketchMinANI takes an ANI in [0, 100]")):
        r = run(binary, ["--ql", lst, "--rl", lst] + args + ["-o", bad])
        assert r.returncode == 1 and b"ERROR, " + msg in r.stderr, (args, r.returncode, r.stderr[-500:])
        assert not os.path.exists(bad) and not os.path.exists(bad + ".sketch")
    few = os.path.join(tmp, "few.txt")
    open(few, "w").write("\n".join(paths[:4]) + "\n")
    for extra in (["--sketchANI"], ["--tree", "--treeFill", "sketch"]):
        r = run(binary, ["--ql", lst, "--rl", few] + extra + ["-o", bad], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 1 and b"is not among the references" in r.stderr and paths[4].encode() in r.stderr, r.stderr[-500:]
        assert b"queries mapped" not in r.stderr and not os.path.exists(bad)
    skf4 = os.path.join(tmp, "few.anisk")
    assert run(binary, ["--ql", few, "--rl", few, "--saveSketch", skf4, "-o", os.path.join(tmp, "save4.out")]).returncode == 0
    r = run(binary, ["--ql", lst, "--refSketch", skf4, "--sketchANI", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"is not among the references" in r.stderr and b"queries mapped" not in r.stderr, r.stderr[-500:]
    # the same file taken in blocks of genomes: refused from its name table, before a block is loaded or anything is mapped
    blocks = {"ANI_CLI_REF_BLOCK_BYTES": "30000", "ANI_CLI_TRACE": "1"}
    r = run(binary, ["--ql", lst, "--refSketch", skf4, "-o", os.path.join(tmp, "blk.out")], blocks)
    assert r.returncode == 0 and b"blocks of genomes per device" in r.stderr and b"reference block 2 of" in r.stderr, r.stderr[-2000:]
    for extra in (["--sketchANI"], ["--tree", "--treeFill", "sketch"]):
        r = run(binary, ["--ql", lst, "--refSketch", skf4] + extra + ["-o", bad], blocks)
        assert r.returncode == 1 and b"is not among the references" in r.stderr and paths[4].encode() in r.stderr, r.stderr[-500:]
        for mark in (b"reference block", b"mapping fragments", b"queries mapped", b"index built", b"devices initialised"):
            assert mark not in r.stderr, mark
        assert not os.path.exists(bad)
    # a subset of the references as queries is fine: the .matrix genomes are all references
    sub = os.path.join(tmp, "sub.out")
    r = run(binary, ["--ql", few, "--rl", lst, "--sketchANI", "--sketchSize", str(size), "--sketchMinANI", "0", "-o", sub])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert len(open(sub + ".sketch").read().splitlines()) == len(pairs)


def test_cli_sketch_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 50000)


@pytest.mark.gpu
def test_cli_sketch_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
