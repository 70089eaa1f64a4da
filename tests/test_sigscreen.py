"""Sketch screening of queries against references (ani_signature_screen, Engine.signature_screen, fastANI --sketchScreen) against the
composition that defines it (include/ani_abi.h, rules 1 - 3): the pairs of ani_signature_pairs over the references followed by the
queries, those of a reference and a query kept at the identity threshold, ordered by identity descending and reference id ascending,
cut at k.  Every comparison is exact: ids, counts, shared, size, identity by bit pattern, and the unused slots.  The expected lists are
always made from engine.signature_pairs over the concatenation or from the numpy pair_expected, never from the call under test and
never from signature_neighbors.  CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library
and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fastani_amd
from fastani_amd.api import NEIGHBOR_DT, AniError
from test_sigdist import identity_expected, make_signatures, pair_expected, two_genera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
STRIP, SHAPE = "ANI_TEST_SIG_STRIP_ROWS", "ANI_TEST_SIG_SCREEN_SHAPE"
STRIPS = (None, 1, 3, 7, 16, 17, 64)       # unset, one row, ragged strips below the square tile, one tile, a tile and a row, more than nQry
UNUSED = np.array((-1, 0, 0, 0.0), dtype=NEIGHBOR_DT)


def set_env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition: rules 2 - 3 over the pairs of the concatenation
# ---------------------------------------------------------------------------------------------------------------------------------
def lists_of(candidates, n_qry, k):
    """{query: [(reference, shared, size, identity float32)]} -> (neighbors, count)"""
    out = np.zeros((n_qry, k), dtype=NEIGHBOR_DT)
    out[:] = UNUSED
    count = np.zeros(n_qry, dtype=np.int32)
    for q in range(n_qry):
        best = sorted(candidates.get(q, []), key=lambda c: (-bits(c[3]), c[0]))[:k]
        count[q] = len(best)
        for i, c in enumerate(best):
            out[q, i] = c
    return out, count


def expected(pairs, n_ref, n_qry, k, min_identity):
    """the lists of the queries [0, n_qry) from a SIGPAIR_DT array over references + queries; also the candidates per query"""
    low = bits(0.0 if min_identity == 0 else min_identity)
    cand = {}
    for p in pairs:
        a, b = int(p["a"]), int(p["b"])
        if a < n_ref <= b < n_ref + n_qry and bits(p["identity"]) >= low:
            cand.setdefault(b - n_ref, []).append((a, int(p["shared"]), int(p["size"]), p["identity"]))
    return lists_of(cand, n_qry, k), [len(cand.get(q, [])) for q in range(n_qry)]


def expected_numpy(ref, ref_len, qry, qry_len, kmer, k, min_shared, min_identity):
    """the same from pair_expected and identity_expected alone"""
    size = ref.shape[1]
    low = bits(0.0 if min_identity == 0 else min_identity)
    cand, shareds = {}, set()
    for q in range(len(qry)):
        for r in range(len(ref)):
            sh, sz = pair_expected(ref[r, :ref_len[r]], qry[q, :qry_len[q]], size)
            shareds.add(sh)
            w = identity_expected(sh, sz, kmer)
            if sh >= min_shared and bits(w) >= low:
                cand.setdefault(q, []).append((r, sh, sz, w))
    return lists_of(cand, len(qry), k), shareds


def same(got, want):
    (nb, count), (wnb, wcount) = got, want
    assert nb.dtype == NEIGHBOR_DT and count.dtype == np.int32 and nb.shape == wnb.shape and count.shape == wcount.shape
    assert np.array_equal(count, wcount), (count, wcount)
    for f in ("neighbor", "shared", "size"):
        assert np.array_equal(nb[f], wnb[f]), f
    assert np.array_equal(nb["identity"].view(np.uint32), wnb["identity"].view(np.uint32))
    for q in range(len(count)):
        assert (nb[q, count[q]:] == UNUSED).all()


def strips_of(strip, rows):
    return 0 if rows == 0 else 1 if strip is None else -(-rows // min(strip, rows))


def small_data():
    """40 references and 23 queries of size 16 from a small pool: empty and full signatures on both sides; query 2 is reference 11, query 7 is
    empty"""
    rng = np.random.default_rng(41)
    sets = [rng.choice(60, size=int(rng.integers(0, 26)), replace=False) * 70001 for _ in range(63)]
    sets[40 + 2] = sets[11]
    sets[40 + 7] = sets[0][:0]                                                       # (the draw leaves no query empty)
    sig, length = make_signatures(sets, 16)
    assert (length[:40] == 0).any() and (length[:40] == 16).any() and (length[40:] == 0).any() and (length[40:] == 16).any()
    assert length[11] > 0
    return sig, length


def composition_small(engine, monkeypatch):
    sig, length = small_data()
    n_ref, n_qry = 40, 23
    ref, ref_len, qry, qry_len = sig[:n_ref], length[:n_ref], sig[n_ref:], length[n_ref:]
    set_env(monkeypatch, STRIP, None)
    set_env(monkeypatch, SHAPE, None)
    fewer = more = False
    for kmer, idents in ((16, (0.0, 70.0, 100.0, -0.0)), (9, (0.0, 70.0))):
        for ms in (1, 3):
            pairs = engine.signature_pairs(sig, length, kmer, ms)
            for k in (1, 3, 8, 39, 64):
                for mi in idents:
                    want, cands = expected(pairs, n_ref, n_qry, k, mi)
                    got = engine.signature_screen(ref, ref_len, qry, qry_len, kmer, k, ms, mi)
                    same(got, want)
                    assert engine.signature_screen_strips() == 1
                    fewer |= any(c < k for c in cands)
                    more |= any(c > k for c in cands)
                    if mi <= 0:                                       # the copied row: its reference leads at 100 (ties: the lowest id at 100)
                        nb, count = got
                        first = min(r for r in range(n_ref) if length[r] == length[11] and (sig[r] == sig[11]).all())
                        assert count[2] >= 1 and nb[2, 0]["neighbor"] == first and bits(nb[2, 0]["identity"]) == bits(100.0)
                        assert nb[2, 0]["shared"] == nb[2, 0]["size"] == length[11]
    assert fewer and more
    # the numpy restatement agrees with the pairs of the engine
    same(expected_numpy(ref, ref_len, qry, qry_len, 16, 8, 1, 0.0)[0], expected(engine.signature_pairs(sig, length, 16, 1), n_ref, n_qry, 8, 0.0)[0])


def test_composition_small_cpu_build(emu_engine, monkeypatch):
    composition_small(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_composition_small_gpu(gpu_engine, monkeypatch):
    composition_small(gpu_engine, monkeypatch)


def strips_and_shapes(engine, monkeypatch):
    """every strip height x every prefix of the queries x three reference counts (none a multiple of a tile's references), under the
    shape the strip height selects and under either forced shape: one result"""
    sig, length = small_data()
    more = make_signatures([np.arange(i, i + 9) * 70001 for i in range(25)], 16)
    all_ref, all_len = np.concatenate([sig[:40], more[0]]), np.concatenate([length[:40], more[1]])
    qry, qry_len = sig[40:], length[40:]
    turn, tiles = 0, set()
    for n_ref in (1, 40, 65):
        ref, ref_len = all_ref[:n_ref], all_len[:n_ref]
        set_env(monkeypatch, STRIP, None)
        pairs = engine.signature_pairs(np.concatenate([ref, qry]), np.concatenate([ref_len, qry_len]), 16, 1)
        for n_qry in (1, 4, 5, 16, 17, 23):
            for strip in STRIPS:
                k, mi = (1, 3, 8, 39, 64)[turn % 5], (0.0, 70.0, 100.0)[turn % 3]
                turn += 1
                want, _ = expected(pairs, n_ref, n_qry, k, mi)
                for shape in (None, "square", "thin"):
                    set_env(monkeypatch, STRIP, strip)
                    set_env(monkeypatch, SHAPE, shape)
                    same(engine.signature_screen(ref, ref_len, qry[:n_qry], qry_len[:n_qry], 16, k, 1, mi), want)
                    assert engine.signature_screen_strips() == strips_of(strip, n_qry), (strip, n_qry)
                    tile = engine.signature_screen_tile()
                    if shape is None:                                  # the last strip's height decides: below the 16 of this pitch, the thin tile
                        h = n_qry if strip is None else min(strip, n_qry)
                        last = n_qry - (n_qry - 1) // h * h
                        assert tile == ((1, 64) if last < 16 else (16, 16)), (tile, strip, n_qry)
                    else:
                        assert tile == ((1, 64) if shape == "thin" else (16, 16))
                    tiles.add((shape, tile))
    assert {t for s, t in tiles if s is None} == {(1, 64), (16, 16)}                 # both shapes ran unforced


def test_strips_and_shapes_cpu_build(emu_engine, monkeypatch):
    strips_and_shapes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_strips_and_shapes_gpu(gpu_engine, monkeypatch):
    strips_and_shapes(gpu_engine, monkeypatch)


def pitch_classes(engine, monkeypatch):
    """9 references x 3 queries at a size of every pitch class (<= 256, <= 1024, <= 2048, above): the thin tile by the strip height, the
    square tile of the class forced; against numpy alone"""
    rng = np.random.default_rng(47)
    set_env(monkeypatch, STRIP, None)
    for size, universe, square in ((16, 40, 16), (300, 900, 16), (1100, 4000, 8), (2100, 7000, 4)):
        sets = [rng.choice(universe, size=int(rng.integers(size * 4 // 5, size * 4 // 3)), replace=False) * 500009 for _ in range(12)]
        sets[9] = sets[4]                                                            # query 0 is reference 4
        sets[10] = sets[10][: size // 3]                                             # a short query
        sig, length = make_signatures(sets, size)
        ref, ref_len, qry, qry_len = sig[:9], length[:9], sig[9:], length[9:]
        for k, mi in ((3, 0.0), (11, 70.0)):
            want, shareds = expected_numpy(ref, ref_len, qry, qry_len, 16, k, 1, mi)
            assert len(shareds - {0}) >= 2, shareds
            for shape, tile in ((None, (1, 64)), ("square", (square, square)), ("thin", (1, 64))):
                set_env(monkeypatch, SHAPE, shape)
                same(engine.signature_screen(ref, ref_len, qry, qry_len, 16, k, 1, mi), want)
                assert engine.signature_screen_tile() == tile, (size, shape)


def test_pitch_classes_cpu_build(emu_engine, monkeypatch):
    pitch_classes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_pitch_classes_gpu(gpu_engine, monkeypatch):
    pitch_classes(gpu_engine, monkeypatch)


def ties(engine, monkeypatch):
    """thirty references in three groups of ten with one signature each, and a query of each group's signature: its ten twins at 100
    in reference-id order, then the references of the groups next to its own at the estimate of 3 shared of 8 (groups 0 and 2 share
    nothing), so k cuts inside a run of equal identities"""
    n, size = 30, 8
    base = [np.arange(0, 8), np.arange(5, 13), np.arange(10, 18)]
    ref, ref_len = make_signatures([base[g % 3] * 1000 for g in range(n)], size)
    qry, qry_len = make_signatures([b * 1000 for b in base], size)
    near = identity_expected(3, 8, 16)
    set_env(monkeypatch, STRIP, None)
    pairs = engine.signature_pairs(np.concatenate([ref, qry]), np.concatenate([ref_len, qry_len]), 16, 1)
    for k in (1, 4, 9, 10, 11, 25, 30):
        cand = {q: [(r, 8, 8, np.float32(100.0)) for r in range(n) if r % 3 == q] + [(r, 3, 8, near) for r in range(n) if abs(r % 3 - q) == 1] for q in range(3)}
        direct = lists_of(cand, 3, k)
        same(expected(pairs, n, 3, k, 0.0)[0], direct)
        for strip, shape in ((None, None), (1, None), (2, "square")):
            set_env(monkeypatch, STRIP, strip)
            set_env(monkeypatch, SHAPE, shape)
            nb, count = engine.signature_screen(ref, ref_len, qry, qry_len, 16, k)
            same((nb, count), direct)
            assert count.tolist() == [min(k, 20), min(k, 30), min(k, 20)]                           # the lists stop exactly at k
            for q in range(3):
                row = nb[q, :count[q]]
                run = row["identity"].view(np.uint32)
                assert (np.diff(run.astype(np.int64)) <= 0).all()
                assert all(row["neighbor"][i] < row["neighbor"][i + 1] for i in range(len(row) - 1) if run[i] == run[i + 1])
                assert row["neighbor"][:min(k, 10)].tolist() == [r for r in range(n) if r % 3 == q][:k]


def test_ties_cpu_build(emu_engine, monkeypatch):
    ties(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_ties_gpu(gpu_engine, monkeypatch):
    ties(gpu_engine, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# edges and errors
# ---------------------------------------------------------------------------------------------------------------------------------
def edges_and_errors(engine):
    ref, ref_len = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    qry, qry_len = make_signatures([[2, 3, 4], [7, 8]], 3)
    lib, h = engine.lib, engine.h
    out, cnt = np.zeros(4, dtype=NEIGHBOR_DT), np.full(2, -7, np.int32)
    out[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT)

    def call(n_ref=3, n_qry=2, size=3, kmer=16, ms=1, mi=0.0, k=2, ref_p=ref.ctypes.data, rlen_p=ref_len.ctypes.data, qry_p=qry.ctypes.data,
             qlen_p=qry_len.ctypes.data, out_p=out.ctypes.data, cnt_p=cnt.ctypes.data, ctx=h):
        return lib.ani_signature_screen(ctx, ref_p, rlen_p, n_ref, qry_p, qlen_p, n_qry, size, kmer, ms, ctypes.c_float(mi), k, out_p, cnt_p)

    assert call() == 0 and cnt.tolist() == [2, 0]
    w = identity_expected(2, 3, 16)
    assert out.tolist() == [(1, 3, 3, 100.0), (0, 2, 3, float(w)), (-1, 0, 0, 0.0), (-1, 0, 0, 0.0)]
    assert lib.ani_signature_screen_strips(h) == 1
    # rule 4, one at a time
    for size in (0, -1, 4097):
        assert call(size=size) == -1, size
    for kmer in (0, -3, 17):
        assert call(kmer=kmer) == -1, kmer
    for ms in (0, -1):
        assert call(ms=ms) == -1, ms
    for mi in (-1.0, 100.5, float("nan")):
        assert call(mi=mi) == -1, mi
    for k in (0, -1, 1025):
        assert call(k=k) == -1, k
    assert call(n_ref=-1) == -1 and call(n_qry=-1) == -1
    for null in ("ref_p", "rlen_p", "qry_p", "qlen_p", "out_p", "cnt_p", "ctx"):
        assert call(**{null: None}) == -1, null
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.signature_screen(ref, np.array(bad_len, dtype=np.int32), qry, qry_len, 16, 2)
        assert ex.value.code == -1, bad_len
    for bad_len in ([4, 2], [3, -1]):
        with pytest.raises(AniError) as ex:
            engine.signature_screen(ref, ref_len, qry, np.array(bad_len, dtype=np.int32), 16, 2)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = ref.copy()
        x[1] = bad_row                                                 # a reference that does not ascend
        with pytest.raises(AniError) as ex:
            engine.signature_screen(x, ref_len, qry, qry_len, 16, 2)
        assert ex.value.code == -1, bad_row
        y = qry.copy()
        y[0] = bad_row                                                 # a query that does not ascend
        with pytest.raises(AniError) as ex:
            engine.signature_screen(ref, ref_len, y, qry_len, 16, 2)
        assert ex.value.code == -1, bad_row
    with pytest.raises(AniError) as ex:                                # ... and with no reference to compare it with
        engine.signature_screen(ref[:0], ref_len[:0], np.array([[3, 2, 1]], np.uint32), np.array([3], np.int32), 16, 2)
    assert ex.value.code == -1
    y = qry.copy()
    y[1] = [7, 8, 1]                                                   # beyond the length: not looked at
    same(engine.signature_screen(ref, ref_len, y, qry_len, 16, 2), engine.signature_screen(ref, ref_len, qry, qry_len, 16, 2))
    with pytest.raises(ValueError):                                    # the two sizes must agree
        engine.signature_screen(ref, ref_len, np.zeros((2, 4), np.uint32), qry_len, 16, 2)
    # rule 5: the limits, before anything is read or allocated
    assert call(n_ref=(1 << 30) + 1, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == -4
    assert call(n_qry=(1 << 30) + 1, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == -4
    assert call(n_ref=(1 << 30) + 1, k=0) == -1                        # (the argument checks come first)
    big = np.zeros(2048, dtype=NEIGHBOR_DT)
    assert call(k=1024, out_p=big.ctypes.data) == 0 and big["neighbor"][:3].tolist() == [1, 0, -1]      # the largest k passes
    # rule 6: no queries -> ANI_OK after the scalar checks, nothing read or written, null pointers allowed
    out[:], cnt[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT), -7
    before = (out.copy(), cnt.copy())
    for n_ref in (3, 0):
        assert call(n_ref=n_ref, n_qry=0) == 0
        assert call(n_ref=n_ref, n_qry=0, ref_p=None, rlen_p=None, qry_p=None, qlen_p=None, out_p=None, cnt_p=None) == 0
        assert lib.ani_signature_screen_strips(h) == 0
        assert call(n_ref=n_ref, n_qry=0, k=0) == -1 and call(n_ref=n_ref, n_qry=0, mi=float("nan")) == -1
    assert np.array_equal(out, before[0]) and np.array_equal(cnt, before[1])
    nb, count = engine.signature_screen(ref, ref_len, qry[:0], qry_len[:0], 16, 3)
    assert nb.shape == (0, 3) and nb.dtype == NEIGHBOR_DT and count.shape == (0,)
    # no references -> every count 0, every slot unused; the reference pointers may be null
    assert call(n_ref=0, ref_p=None, rlen_p=None) == 0
    assert cnt.tolist() == [0, 0] and (out == UNUSED).all()
    nb, count = engine.signature_screen(ref[:0], ref_len[:0], qry, qry_len, 16, 5)
    assert count.tolist() == [0, 0] and nb.shape == (2, 5) and (nb == UNUSED).all()
    assert lib.ani_signature_screen_strips(None) == 0


def test_edges_and_errors_cpu_build(emu_engine):
    edges_and_errors(emu_engine)


@pytest.mark.gpu
def test_edges_and_errors_gpu(gpu_engine):
    edges_and_errors(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def run(binary, args, env=None):
    return subprocess.run([binary] + args, capture_output=True, env=dict(os.environ, **(env or {})))


def screen_text(engine, genomes, paths, refs, queries, size, k, min_ani):
    """the .screen file through the API: the signatures of a reference sketch built over each list, then the composition"""
    p = engine.params(16, 3000)
    sigs = []
    for idx in (refs, queries):
        sk = fastani_amd.Sketch(engine, p, [genomes[i] for i in idx])
        sigs.append(sk.signatures(size))
        sk.close()
    (ref, ref_len), (qry, qry_len) = sigs
    pairs = engine.signature_pairs(np.concatenate([ref, qry]), np.concatenate([ref_len, qry_len]), 16, 1)
    (nb, count), _ = expected(pairs, len(refs), len(queries), k, min_ani)
    out = []
    for q, qi in enumerate(queries):
        out += ["%s\t%s\t%s\t%d/%d\n" % (paths[qi], paths[refs[r["neighbor"]]], "%g" % r["identity"], r["shared"], r["size"]) for r in nb[q, :count[q]]] \
            or ["%s\tNA\tNA\tNA\n" % paths[qi]]
    return "".join(out)


def run_cli(binary, engine, tmp, n_len):
    lst, paths, genomes = two_genera(tmp, n_len)
    size = 2000
    sized = ["--sketchSize", str(size), "--sketchMinANI", "0"]

    def lists(name, refs, queries):
        rl, ql = os.path.join(tmp, name + "_r.txt"), os.path.join(tmp, name + "_q.txt")
        open(rl, "w").write("".join(paths[i] + "\n" for i in refs))
        open(ql, "w").write("".join(paths[i] + "\n" for i in queries))
        return rl, ql

    cases = {"disjoint": ([0, 1, 3, 4], [2, 5]), "overlap": ([0, 1, 2, 3], [2, 3, 4, 5]), "all": (list(range(6)), list(range(6)))}
    wants = {}
    for name, (refs, queries) in cases.items():
        rl, ql = lists(name, refs, queries)
        common = ["--ql", ql, "--rl", rl, "--matrix"]
        base, scr = os.path.join(tmp, name + "_base.out"), os.path.join(tmp, name + "_scr.out")
        assert run(binary, common + ["-o", base]).returncode == 0
        r = run(binary, common + ["--sketchScreen", "3"] + sized + ["-o", scr], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert b"sketch screen done" in r.stderr and b"sketch screen written" in r.stderr and b"sketch pairs compared" not in r.stderr
        # without the option every file is as before; with it, every other file
        assert not os.path.exists(base + ".screen") and not os.path.exists(scr + ".neighbors") and not os.path.exists(scr + ".sketch")
        for ext in ("", ".matrix"):
            assert open(scr + ext, "rb").read() == open(base + ext, "rb").read(), (name, ext)
        wants[name] = screen_text(engine, genomes, paths, refs, queries, size, 3, 0.0)
        assert open(scr + ".screen").read() == wants[name], name
        assert len(wants[name].splitlines()) > len(queries) and "\tNA\t" not in wants[name]        # every query has relatives among the references
    # a query that is a reference finds itself first, at 100
    first = {}
    for ln in wants["all"].splitlines():
        first.setdefault(ln.split("\t")[0], ln.split("\t")[1:3])
    assert all(first[p] == [p, "100"] for p in paths)
    # the other paths of the command line: two device contexts (the queries' fragment sets in waves), strips of one query, the per-query
    # mapping path with two reference splits, a reference sketch file in blocks of genomes
    rl, ql = lists("disjoint", *cases["disjoint"])
    orl, oql = lists("overlap", *cases["overlap"])
    skf = os.path.join(tmp, "refs.anisk")
    assert run(binary, ["--ql", rl, "--rl", rl, "--saveSketch", skf, "-o", os.path.join(tmp, "save.out")]).returncode == 0
    opt = ["--sketchScreen", "3"] + sized
    for name, args, env, mark, want in (("devices", ["--ql", oql, "--rl", orl, "--devices", "0,0"], {}, b"", "overlap"),
                                        ("strips", ["--ql", oql, "--rl", orl], {STRIP: "1"}, b"", "overlap"),
                                        ("visual", ["--ql", ql, "--rl", rl, "-t", "2", "--visualize"], {}, b"", "disjoint"),
                                        ("blocks", ["--ql", ql, "--refSketch", skf], {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, b"blocks of genomes per device", "disjoint")):
        o = os.path.join(tmp, name + ".out")
        r = run(binary, args + opt + ["-o", o], env)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert mark in r.stderr
        assert open(o + ".screen").read() == wants[want], name
    assert open(os.path.join(tmp, "blocks.out"), "rb").read() == open(os.path.join(tmp, "disjoint_base.out"), "rb").read()
    # default size and threshold, --sketchMinANI with this option alone; one genome of the second genus against the first at 99: NA
    grl, gql = lists("genus", [0, 1, 2], [3, 1])
    for args, min_ani, k in (([], 70.0, 2), (["--sketchMinANI", "99"], 99.0, 2)):
        o = os.path.join(tmp, "genus%d.out" % len(args))
        r = run(binary, ["--ql", gql, "--rl", grl, "--sketchScreen", str(k)] + args + ["-o", o])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        want = screen_text(engine, genomes, paths, [0, 1, 2], [3, 1], 1000, k, min_ani)
        assert open(o + ".screen").read() == want
    assert want.splitlines()[0] == "%s\tNA\tNA\tNA" % paths[3] and want.splitlines()[1].split("\t")[:3] == [paths[1], paths[1], "100"]
    # a query absent from the references stops the run only beside an option that compares the references
    bad = os.path.join(tmp, "bad.out")
    r = run(binary, ["--ql", ql, "--rl", rl, "--sketchScreen", "2", "--sketchNeighbors", "2", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"is not among the references" in r.stderr and paths[2].encode() in r.stderr, r.stderr[-500:]
    assert b"ERROR, --sketchANI, --sketchNeighbors and --treeFill sketch compare the reference genomes: query " in r.stderr
    assert b"devices initialised" not in r.stderr and not os.path.exists(bad) and not os.path.exists(bad + ".screen")
    for k in ("0", "1025"):
        r = run(binary, ["--ql", ql, "--rl", rl, "--sketchScreen", k, "-o", bad])
        assert r.returncode == 1 and b"ERROR, --sketchScreen takes a count from 1 to 1024" in r.stderr, (k, r.stderr[-300:])
    assert not os.path.exists(bad)


def test_cli_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 8000)


@pytest.mark.gpu
def test_cli_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
