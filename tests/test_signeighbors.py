"""Sketch nearest neighbours (ani_signature_neighbors, Engine.signature_neighbors, fastANI --sketchNeighbors) against the composition that
defines them (include/ani_abi.h, rules 1 - 7): the pairs of ani_signature_pairs, kept at the identity threshold, ordered by identity
descending and neighbour id ascending, cut at k.  Every comparison is exact: ids, counts, shared, size, identity by bit pattern, and
the unused slots.  The expected lists are always made from engine.signature_pairs or pair_expected, never from the call under test.
CPU: the tests/emu build of the library and of the command line; GPU (-m gpu): the product library and fastani_amd/fastANI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from fastani_amd.api import NEIGHBOR_DT, AniError
from test_cluster import read_matrix
from test_sigdist import identity_expected, make_signatures, pair_expected, two_genera
from test_tree_single_sketch import grouped_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
STRIP = "ANI_TEST_SIG_STRIP_ROWS"
STRIPS = (None, 1, 7, 16, 17, 64)          # unset, one row, a ragged strip, one tile, a tile and a row, more than n


def set_strip(monkeypatch, rows):
    if rows is None:
        monkeypatch.delenv(STRIP, raising=False)
    else:
        monkeypatch.setenv(STRIP, str(rows))


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition: rules 2 - 6 over the pairs
# ---------------------------------------------------------------------------------------------------------------------------------
def lists_of(candidates, k, begin, end):
    """{genome: [(neighbour, shared, size, identity float32)]} -> (neighbors, count) of rules 3 - 6"""
    out = np.zeros((end - begin, k), dtype=NEIGHBOR_DT)
    out["neighbor"] = -1
    count = np.zeros(end - begin, dtype=np.int32)
    for g in range(begin, end):
        best = sorted(candidates.get(g, []), key=lambda c: (-bits(c[3]), c[0]))[:k]
        count[g - begin] = len(best)
        for i, c in enumerate(best):
            out[g - begin, i] = c
    return out, count


def expected(pairs, k, min_identity, begin, end):
    """the lists of [begin, end) from a SIGPAIR_DT array"""
    low = bits(0.0 if min_identity == 0 else min_identity)
    cand = {}
    for p in pairs:
        if bits(p["identity"]) >= low:
            a, b = int(p["a"]), int(p["b"])
            cand.setdefault(a, []).append((b, int(p["shared"]), int(p["size"]), p["identity"]))
            cand.setdefault(b, []).append((a, int(p["shared"]), int(p["size"]), p["identity"]))
    return lists_of(cand, k, begin, end), {g: len(c) for g, c in cand.items()}


def same(got, want):
    (nb, count), (wnb, wcount) = got, want
    assert nb.dtype == NEIGHBOR_DT and count.dtype == np.int32 and nb.shape == wnb.shape and count.shape == wcount.shape
    assert np.array_equal(count, wcount), (count, wcount)
    for f in ("neighbor", "shared", "size"):
        assert np.array_equal(nb[f], wnb[f]), f
    assert np.array_equal(nb["identity"].view(np.uint32), wnb["identity"].view(np.uint32))


def strips_of(strip, rows):
    return 0 if rows == 0 else 1 if strip is None else -(-rows // min(strip, rows))


def equals_composition(engine, monkeypatch):
    rng = np.random.default_rng(41)
    n, size = 40, 16
    sig, length = make_signatures([rng.choice(60, size=int(rng.integers(0, 26)), replace=False) * 70001 for _ in range(n)], size)
    assert (length == 0).any() and (length == size).any()
    ks, shareds, idents, ranges = (1, 3, 8, 39, 64), (1, 3), (0.0, 70.0, 100.0), ((0, 40), (5, 23), (39, 40), (7, 7))
    set_strip(monkeypatch, None)
    pairs = {ms: engine.signature_pairs(sig, length, 16, ms) for ms in shareds}
    fewer = more = False
    # every k, minShared and minIdentity at the default strip height, all rows
    for k in ks:
        for ms in shareds:
            for mi in idents:
                want, cands = expected(pairs[ms], k, mi, 0, n)
                same(engine.signature_neighbors(sig, length, 16, k, ms, mi), want)
                assert engine.signature_neighbors_strips() == 1
                fewer |= any(cands.get(g, 0) < k for g in range(n))
                more |= any(c > k for c in cands.values())
    assert fewer and more
    # every strip height with every row range; k, minShared and minIdentity take turns
    turn = 0
    for strip in STRIPS:
        for begin, end in ranges:
            k, ms, mi = ks[turn % len(ks)], shareds[turn % len(shareds)], idents[turn % len(idents)]
            turn += 1
            set_strip(monkeypatch, strip)
            want, _ = expected(pairs[ms], k, mi, begin, end)
            same(engine.signature_neighbors(sig, length, 16, k, ms, mi, rows=(begin, end)), want)
            assert engine.signature_neighbors_strips() == strips_of(strip, end - begin), (strip, begin, end)
    # -0.0 is 0; a k-mer size that moves the estimates
    set_strip(monkeypatch, 7)
    same(engine.signature_neighbors(sig, length, 16, 8, 1, -0.0), expected(pairs[1], 8, 0.0, 0, n)[0])
    p9 = engine.signature_pairs(sig, length, 9, 1)
    same(engine.signature_neighbors(sig, length, 9, 5, 1, 40.0), expected(p9, 5, 40.0, 0, n)[0])


def test_equals_composition_cpu_build(emu_engine, monkeypatch):
    equals_composition(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_equals_composition_gpu(gpu_engine, monkeypatch):
    equals_composition(gpu_engine, monkeypatch)


def ties(engine, monkeypatch):
    """three groups of ten with one signature each: a genome has its 9 twins at 100, and the 10 genomes of each group next to its own
    at the estimate of 3 shared of 8 (groups 0 and 2 share nothing), so the k-th place falls inside a run of equal identities"""
    n, size = 30, 8
    base = [np.arange(0, 8), np.arange(5, 13), np.arange(10, 18)]
    sig, length = make_signatures([base[g % 3] * 1000 for g in range(n)], size)
    set_strip(monkeypatch, None)
    pairs = engine.signature_pairs(sig, length, 16, 1)
    near = identity_expected(3, 8, 16)
    for k in (1, 4, 9, 10, 29):
        # stated directly: the twins ascending, then the genomes of the groups next to one's own, ascending
        cand = {}
        for g in range(n):
            twins = [(b, 8, 8, np.float32(100.0)) for b in range(n) if b != g and b % 3 == g % 3]
            others = [(b, 3, 8, near) for b in range(n) if abs(b % 3 - g % 3) == 1]
            cand[g] = twins + others
        direct = lists_of(cand, k, 0, n)
        want, _ = expected(pairs, k, 0.0, 0, n)
        same(want, direct)
        for strip in (None, 1, 7):
            set_strip(monkeypatch, strip)
            nb, count = engine.signature_neighbors(sig, length, 16, k)
            same((nb, count), want)
            assert count.tolist() == [min(k, 29 if g % 3 == 1 else 19) for g in range(n)]              # the lists stop exactly at k
            for g in range(n):
                row = nb[g, :count[g]]
                run = row["identity"].view(np.uint32)
                assert (np.diff(run.astype(np.int64)) <= 0).all()
                assert all(row["neighbor"][i] < row["neighbor"][i + 1] for i in range(len(row) - 1) if run[i] == run[i + 1])
                assert (nb[g, count[g]:] == np.array((-1, 0, 0, 0.0), dtype=NEIGHBOR_DT)).all()


def test_ties_cpu_build(emu_engine, monkeypatch):
    ties(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_ties_gpu(gpu_engine, monkeypatch):
    ties(gpu_engine, monkeypatch)


def tile_shapes(engine, monkeypatch):
    """the tile edges 8, 4 and 16 (small LDS, ragged last tile), each under strips of one row and of a tile and a row"""
    rng = np.random.default_rng(43)
    for size, n, universe, edge in ((1100, 12, 4000, 8), (2100, 6, 7000, 4), (200, 33, 700, 16)):
        sets = [rng.choice(universe, size=int(rng.integers(size * 4 // 5, size * 4 // 3)), replace=False) * 500009 for _ in range(n)]
        sets[1] = sets[0]                                                                             # one pair at 100
        sig, length = make_signatures(sets, size)
        set_strip(monkeypatch, None)
        pairs = engine.signature_pairs(sig, length, 16, 1)
        assert len(pairs) > n
        for strip in (1, edge + 1):
            set_strip(monkeypatch, strip)
            for k, mi in ((3, 0.0), (n + 2, 70.0)):
                same(engine.signature_neighbors(sig, length, 16, k, 1, mi), expected(pairs, k, mi, 0, n)[0])
                assert engine.signature_neighbors_strips() == strips_of(strip, n)


def test_tile_shapes_cpu_build(emu_engine, monkeypatch):
    tile_shapes(emu_engine, monkeypatch)


@pytest.mark.gpu
def test_tile_shapes_gpu(gpu_engine, monkeypatch):
    tile_shapes(gpu_engine, monkeypatch)


def degenerate_sizes(engine):
    nb, count = engine.signature_neighbors(np.zeros((0, 5), np.uint32), np.zeros(0, np.int32), 16, 3)
    assert nb.shape == (0, 3) and nb.dtype == NEIGHBOR_DT and count.shape == (0,)
    nb, count = engine.signature_neighbors(np.array([[1, 2, 3, 0, 0]], np.uint32), np.array([3], np.int32), 16, 3)
    assert count.tolist() == [0] and nb.tolist() == [[(-1, 0, 0, 0.0)] * 3]
    sig, length = make_signatures([[1, 2, 3, 4], [3, 4, 5]], 5)
    sh, sz = pair_expected(sig[0, :4], sig[1, :3], 5)
    assert (sh, sz) == (2, 5)
    w = identity_expected(sh, sz, 16)
    nb, count = engine.signature_neighbors(sig, length, 16, 2)
    assert count.tolist() == [1, 1] and nb["neighbor"].tolist() == [[1, -1], [0, -1]] and nb["shared"].tolist() == [[2, 0], [2, 0]]
    assert nb["size"].tolist() == [[5, 0], [5, 0]] and nb["identity"].view(np.uint32).tolist() == [[bits(w), 0], [bits(w), 0]]
    nb, count = engine.signature_neighbors(sig, length, 16, 2, min_shared=3)
    assert count.tolist() == [0, 0] and (nb["neighbor"] == -1).all()
    nb, count = engine.signature_neighbors(sig, length, 16, 1, rows=(1, 2))
    assert count.tolist() == [1] and nb.tolist() == [[(0, 2, 5, float(w))]]


def test_degenerate_sizes_cpu_build(emu_engine):
    degenerate_sizes(emu_engine)


@pytest.mark.gpu
def test_degenerate_sizes_gpu(gpu_engine):
    degenerate_sizes(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_errors(engine):
    sig, length = make_signatures([[1, 2, 3], [2, 3, 4], [9]], 3)
    lib, h = engine.lib, engine.h
    out, cnt = np.full(6, -7, dtype=NEIGHBOR_DT), np.full(3, -7, np.int32)

    def call(n=3, size=3, kmer=16, ms=1, mi=0.0, k=2, begin=0, end=3, sig_p=sig.ctypes.data, len_p=length.ctypes.data, out_p=out.ctypes.data,
             cnt_p=cnt.ctypes.data, ctx=h):
        return lib.ani_signature_neighbors(ctx, sig_p, len_p, n, size, kmer, ms, ctypes.c_float(mi), k, begin, end, out_p, cnt_p)

    assert call() == 0 and cnt.tolist() == [1, 1, 0]
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
    for begin, end in ((-1, 2), (2, 1), (0, 4), (4, 4)):
        assert call(begin=begin, end=end) == -1, (begin, end)
    assert call(n=-1, begin=0, end=0) == -1
    assert call(sig_p=None) == -1 and call(len_p=None) == -1 and call(out_p=None) == -1 and call(cnt_p=None) == -1 and call(ctx=None) == -1
    assert call(n=(1 << 30) + 1) == -4                                 # the limit, before anything is read or allocated
    big = np.zeros(1024, dtype=NEIGHBOR_DT)
    assert call(k=1024, end=1, out_p=big.ctypes.data) == 0 and big["neighbor"][:2].tolist() == [1, -1]      # the largest k passes
    for bad_len in ([3, 4, 1], [3, -1, 1]):
        with pytest.raises(AniError) as ex:
            engine.signature_neighbors(sig, np.array(bad_len, dtype=np.int32), 16, 2)
        assert ex.value.code == -1, bad_len
    for bad_row in ([3, 2, 1], [1, 1, 2], [1, 2, 2]):
        x = sig.copy()
        x[1] = bad_row
        with pytest.raises(AniError) as ex:
            engine.signature_neighbors(x, length, 16, 2)
        assert ex.value.code == -1, bad_row
    x = sig.copy()
    x[2] = [9, 9, 1]                                                   # beyond the length: not looked at
    same(engine.signature_neighbors(x, length, 16, 2), engine.signature_neighbors(sig, length, 16, 2))
    # an empty range or no genomes: ANI_OK after the scalar checks, nothing read or written, null pointers allowed
    out[:], cnt[:] = np.array((-7, -7, -7, -7.0), dtype=NEIGHBOR_DT), -7
    before = (out.copy(), cnt.copy())
    for n, begin, end in ((3, 0, 0), (3, 2, 2), (3, 3, 3), (0, 0, 0)):
        assert call(n=n, begin=begin, end=end) == 0
        assert call(n=n, begin=begin, end=end, sig_p=None, len_p=None, out_p=None, cnt_p=None) == 0
        assert lib.ani_signature_neighbors_strips(h) == 0
        assert call(n=n, begin=begin, end=end, k=0) == -1 and call(n=n, begin=begin, end=end, mi=float("nan")) == -1
    assert np.array_equal(out, before[0]) and np.array_equal(cnt, before[1])
    assert lib.ani_signature_neighbors_strips(None) == 0


def test_errors_cpu_build(emu_engine):
    argument_errors(emu_engine)


@pytest.mark.gpu
def test_errors_gpu(gpu_engine):
    argument_errors(gpu_engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# above the ceiling of the pair step
# ---------------------------------------------------------------------------------------------------------------------------------
def grouped_expected(n, k, begin, end):
    """grouped_input's lists in closed form: groups of three, members 0 and 1 share 2 of 4, member 2 shares 1 of 4 with both (a tie that
    the id resolves); the members of every fifth group are identical; nothing is shared between groups"""
    w = {s: identity_expected(s, 4, 16) for s in (1, 2, 4)}
    out = np.zeros((end - begin, k), dtype=NEIGHBOR_DT)
    out["neighbor"] = -1
    shared = {(0, 1): 2, (0, 2): 1, (1, 2): 1}
    for g in range(begin, end):
        first, member = g // 3 * 3, g % 3
        cand = []
        for other in range(3):
            if other != member:
                s = 4 if (g // 3) % 5 == 0 else shared[(min(member, other), max(member, other))]
                cand.append((first + other, s, 4, w[s]))
        for i, c in enumerate(sorted(cand, key=lambda c: (-bits(c[3]), c[0]))[:k]):
            out[g - begin, i] = c
    return out, np.full(end - begin, min(k, 2), dtype=np.int32)


def test_grouped_closed_form():
    """the closed form against the restatement of the rules, on the first groups"""
    sig, length, _ = grouped_input(66000)
    for g0 in (0, 3):                                                  # an identical group and a mixed one
        for a in range(g0, g0 + 3):
            want, _ = grouped_expected(66000, 2, a, a + 1)
            cand = []
            for b in range(g0, g0 + 3):
                if b != a:
                    sh, sz = pair_expected(sig[a], sig[b], 4)
                    cand.append((b, sh, sz, identity_expected(sh, sz, 16)))
            assert pair_expected(sig[a], sig[(g0 + 3) % 66000 + 1], 4)[0] == 0
            same(lists_of({a: cand}, 2, a, a + 1), (want, np.array([2], dtype=np.int32)))


@pytest.mark.gpu
def test_above_the_old_ceiling_gpu(gpu_engine, monkeypatch):
    n = 66000
    sig, length, _ = grouped_input(n)
    set_strip(monkeypatch, None)
    got = gpu_engine.signature_neighbors(sig, length, 16, 2)
    print("all rows, k = 2: %d strips" % gpu_engine.signature_neighbors_strips())
    same(got, grouped_expected(n, 2, 0, n))
    set_strip(monkeypatch, 256)
    got = gpu_engine.signature_neighbors(sig, length, 16, 1, rows=(65000, 66000))
    assert gpu_engine.signature_neighbors_strips() == 4
    same(got, grouped_expected(n, 1, 65000, 66000))
    # the pair step keeps its ceiling
    with pytest.raises(AniError) as ex:
        gpu_engine.signature_pairs(sig, length, 16, 1)
    assert ex.value.code == -4


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def run(binary, args, env=None):
    return subprocess.run([binary] + args, capture_output=True, env=dict(os.environ, **(env or {})))


def neighbors_from_sketch(sketch_text, names, k, min_ani):
    """the .neighbors file from the lines of a .sketch file written at threshold 0: both directions of each line, ordered by the bits
    of identity_expected(shared, size, 16) descending and the .matrix index ascending, the estimate text taken from the line"""
    index = {name: i for i, name in enumerate(names)}
    cand = {i: [] for i in range(len(names))}
    for ln in sketch_text.splitlines():
        a, b, est, frac = ln.split("\t")
        shared, size = (int(x) for x in frac.split("/"))
        w = identity_expected(shared, size, 16)
        if bits(w) >= bits(min_ani):
            cand[index[a]].append((-bits(w), index[b], est, frac))
            cand[index[b]].append((-bits(w), index[a], est, frac))
    out = []
    for i, name in enumerate(names):
        best = sorted(cand[i])[:k]
        out += ["%s\t%s\t%s\t%s\n" % (name, names[j], est, frac) for _, j, est, frac in best] or ["%s\tNA\tNA\tNA\n" % name]
    return "".join(out)


def run_cli(binary, tmp, n_len):
    lst, paths, _ = two_genera(tmp, n_len)
    common = ["--ql", lst, "--rl", lst, "--matrix"]
    sized = ["--sketchSize", "2000", "--sketchMinANI", "0"]
    base, nb, sk = (os.path.join(tmp, x + ".out") for x in ("base", "nb", "sk"))
    assert run(binary, common + ["-o", base]).returncode == 0
    r = run(binary, common + ["--sketchNeighbors", "3"] + sized + ["-o", nb], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"sketch neighbours found" in r.stderr and b"sketch neighbours written" in r.stderr and b"sketch pairs compared" not in r.stderr
    assert run(binary, common + ["--sketchANI"] + sized + ["-o", sk]).returncode == 0
    # without the option every file is as before; with it, every other file
    assert not os.path.exists(base + ".neighbors") and not os.path.exists(sk + ".neighbors") and not os.path.exists(nb + ".sketch")
    for ext in ("", ".matrix"):
        assert open(nb + ext, "rb").read() == open(base + ext, "rb").read(), ext
    names, _ = read_matrix(nb + ".matrix")
    assert names == paths
    sketch_text = open(sk + ".sketch").read()
    want = neighbors_from_sketch(sketch_text, names, 3, 0.0)
    got = open(nb + ".neighbors").read()
    assert got == want
    assert len(want.splitlines()) > 12 and "\tNA\tNA\tNA\n" not in want                        # inside the genera and across
    # a threshold only the closest pair passes: its two genomes name each other, everyone else has the NA line
    best = max(identity_expected(*(int(x) for x in ln.split("\t")[3].split("/")), 16) for ln in sketch_text.splitlines())
    high = os.path.join(tmp, "high.out")
    r = run(binary, common + ["--sketchNeighbors", "3", "--sketchSize", "2000", "--sketchMinANI", repr(float(best) - 0.001), "-o", high])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want_high = neighbors_from_sketch(sketch_text, names, 3, np.float32(float(best) - 0.001))
    assert open(high + ".neighbors").read() == want_high
    assert want_high.count("\tNA\tNA\tNA\n") >= 1 and len(want_high.splitlines()) > want_high.count("\tNA\tNA\tNA\n")
    # the other paths of the command line: a reference sketch file in blocks of genomes, two device contexts, strips of two rows
    skf = os.path.join(tmp, "refs.anisk")
    assert run(binary, ["--ql", lst, "--rl", lst, "--saveSketch", skf, "-o", os.path.join(tmp, "save.out")]).returncode == 0
    opt = ["--sketchNeighbors", "3"] + sized
    for name, args, env, mark in (("blocks", ["--ql", lst, "--refSketch", skf, "--matrix"], {"ANI_CLI_REF_BLOCK_BYTES": "30000"}, b"blocks of genomes per device"),
                                  ("devices", common + ["--devices", "0,0"], {}, b""), ("strips", common, {STRIP: "2"}, b"")):
        o = os.path.join(tmp, name + ".out")
        r = run(binary, args + opt + ["-o", o], env)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        assert mark in r.stderr
        assert open(o + ".neighbors").read() == want, name
    # with --sketchANI and a tree beside it: the same .neighbors, the same .sketch
    both = os.path.join(tmp, "both.out")
    r = run(binary, common + ["--sketchANI", "--tree", "--treeMethod", "single", "--treeFill", "sketch"] + opt + ["-o", both])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(both + ".neighbors").read() == want and open(both + ".sketch").read() == sketch_text
    # refusals
    bad = os.path.join(tmp, "bad.out")
    for k in ("0", "1025", "-3", "x"):
        r = run(binary, common + ["--sketchNeighbors", k, "-o", bad])
        assert r.returncode == 1 and b"ERROR, --sketchNeighbors takes a count from 1 to 1024" in r.stderr, (k, r.stderr[-300:])
    for args, msg in ((["--sketchSize", "500"], b"ERROR, --sketchSize needs --sketchANI or --treeFill sketch"),
                      (["--sketchMinANI", "80"], b"ERROR, --sketchMinANI needs --sketchANI")):
        r = run(binary, common + args + ["-o", bad])
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr[-300:])
    few = os.path.join(tmp, "few.txt")
    open(few, "w").write("\n".join(paths[:4]) + "\n")
    r = run(binary, ["--ql", lst, "--rl", few, "--sketchNeighbors", "2", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and b"is not among the references" in r.stderr and paths[4].encode() in r.stderr, r.stderr[-500:]
    assert b"devices initialised" not in r.stderr
    assert not os.path.exists(bad) and not os.path.exists(bad + ".neighbors")


def ceiling(binary, tmp):
    """65 537 references: the option alone passes the ceiling check and goes on to the next check of the same function, where a query
    outside the references ends the run; with --sketchANI beside it the pair step's refusal stays"""
    p = os.path.join(tmp, "g.fa")
    open(p, "w").write(">c\nACGT\n")
    names = [os.path.join(tmp, "x%d.fa" % i) for i in range(65537)]
    for x in names:
        os.symlink(p, x)
    many, one, other = os.path.join(tmp, "many.txt"), os.path.join(tmp, "one.txt"), os.path.join(tmp, "other.txt")
    open(many, "w").write("\n".join(names) + "\n")
    open(one, "w").write(names[0] + "\n")
    open(other, "w").write(p + "\n")
    bad = os.path.join(tmp, "bad.out")
    msg = b"ERROR, --sketchANI and --treeFill sketch take at most 65536 genomes, this run has 65537"
    r = run(binary, ["--ql", other, "--rl", many, "--sketchNeighbors", "2", "-o", bad], {"ANI_CLI_TRACE": "1"})
    assert r.returncode == 1 and msg not in r.stderr and b"is not among the references" in r.stderr and b"devices initialised" not in r.stderr, r.stderr[-300:]
    for extra in (["--sketchANI"], ["--tree", "--treeFill", "sketch"]):
        r = run(binary, ["--ql", one, "--rl", many, "--sketchNeighbors", "2"] + extra + ["-o", bad], {"ANI_CLI_TRACE": "1"})
        assert r.returncode == 1 and msg in r.stderr and b"devices initialised" not in r.stderr, (extra, r.stderr[-300:])
    assert not os.path.exists(bad)


def test_cli_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), str(tmp_path), 50000)


def test_cli_ceiling_cpu_build(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    ceiling(os.path.join(EMU, "fastANI_emu"), str(tmp_path))


@pytest.mark.gpu
def test_cli_gpu(tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    for sub in ("a", "b"):
        os.mkdir(os.path.join(str(tmp_path), sub))
    run_cli(binary, os.path.join(str(tmp_path), "a"), 200000)
    ceiling(binary, os.path.join(str(tmp_path), "b"))
