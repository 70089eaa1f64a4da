"""Timings of the whole-genome sketch ANI on the GPU: ani_sketch_signatures on a sketch of synthetic genomes
and ani_signature_pairs on synthetic signatures, at s = 1000.  Both calls return after their last device-to-host copy, so the wall
clock around them includes uploads, kernels and read-back (for the pairs: the host arithmetic of the identities too).

    python tools/sketch_probe.py                 1 000 / 10 000 / 65 536 genomes, 1 warm-up + 3 timed calls each (median reported)
    python tools/sketch_probe.py --only 1000     one genome count (e.g. under rocprofv3)
    python tools/sketch_probe.py --reps 1        timed calls per case (default 3)
    python tools/sketch_probe.py --min-shared 1  the minShared of the pair call (default: above every pair, so no row comes back
                                                 and the time is the comparison's; with 1 the read-back of the rows is included)
    python tools/sketch_probe.py --neighbors     ani_signature_neighbors instead, at 1 000 / 10 000 / 65 536 /
                                                 90 000 genomes, minShared 1, minIdentity 0, --k neighbours (default 10): the call, its
                                                 strips and, up to --compose-max genomes (default 10 000: beyond it the pair rows no
                                                 longer fit a host comfortably, 43 GB at 65 536), ani_signature_pairs at minShared 1
                                                 plus a numpy top-k over its rows, timed and compared with the call's lists
    python tools/sketch_probe.py --screen        ani_signature_screen at 1 / 16 / 1 000 queries x 10 000 references,
                                                 minShared 1, minIdentity 0, --k references (default 10): the call under the tile shape
                                                 its strip height selects and under either forced shape, its strips and tile, and the
                                                 route without it: ani_signature_neighbors over references + queries for the query rows
                                                 at k = 1024, cut to the references on the host; lists compared.  Every line: min .. max
                                                 of the timed calls, by the wall clock and by HIP events around the call
    python tools/sketch_probe.py --screen --contain query|reference|max
                                                 ani_signature_screen_contain in that mode beside
                                                 ani_signature_screen on the same signatures, query counts and tile shapes: min .. max
                                                 and median of the timed calls by HIP events, the merge steps of both rules replayed on
                                                 the host (on a sample of pairs for the larger counts), steps/s, and the time per step
                                                 of the new call over that of the existing one
    python tools/sketch_probe.py --cluster T     ani_signature_cluster at the threshold T, at 10 000 and 90 000
                                                 genomes in families of ten (a tenth of the genomes are representatives at any T
                                                 between 0 and about 97), minShared 1: the call, min .. max and median by HIP events
                                                 and by the wall clock, and its stats call (strips, representatives, cells merged,
                                                 resolve steps); up to --compose-max genomes the composition ani_signature_pairs at
                                                 minShared 1 + ani_cluster_greedy over its rows on the same signatures, timed the same
                                                 way and compared with the call's result
    python tools/sketch_probe.py --cluster T --contain max
                                                 ani_signature_cluster_contain on the same genomes: the call,
                                                 the same call with ANI_TEST_SIG_CLUSTER_TRI=0 (every strip's own block walked in
                                                 full instead of from its upper triangle) and ani_signature_cluster under the Mash
                                                 estimate, taken in turns; min .. max and median of each by HIP events and by the wall
                                                 clock, the stats call of each, and the results of the first two compared
    python tools/sketch_probe.py --graph T [--contain max]
                                                 ani_signature_graph at the threshold T, at 10 000 and 90 000
                                                 genomes in families of ten, minShared 1, all rows in one call, under the Mash estimate
                                                 or with --contain max the containment estimate: min .. max and median by HIP events and
                                                 by the wall clock, its strips and its kept pairs; under the Mash estimate and up to
                                                 --compose-max genomes the composition ani_signature_pairs at minShared 1 + a numpy
                                                 filter by identity bits on the same signatures in the same process, timed the same way
                                                 and compared with the call's records

Signatures for the pair call: every genome draws its values from a universe of 6 000 with a density of its own and keeps the 1 000
smallest, so pairs stop anywhere between a few hundred and the full 1 000 union elements.  Merge steps are counted by replaying the
rule of k_sigpair_merge (kernels/sigdist.hpp) on the host, on a sample of pairs for the larger counts, and scaled to all pairs.
Genomes for the signature call: ani_synth_packed, 200 / 50 / 20 kb each for the three counts (a 20 kb genome has 1 600 minimizers).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 1000
GENOME_LEN = {1000: 200000, 10000: 50000, 65536: 20000}


def synthetic_signatures(rng, n, size=SIZE, universe=6000, step=700000):
    sig = np.zeros((n, size), dtype=np.uint32)
    length = np.zeros(n, dtype=np.int32)
    for g in range(n):
        s = np.flatnonzero(rng.random(universe) < rng.uniform(0.05, 0.7))[:size]
        sig[g, :len(s)] = s.astype(np.uint32) * np.uint32(step)
        length[g] = len(s)
    return sig, length


def merge_steps(x, y, size):
    """steps of the two-pointer walk: union elements taken until `size` of them or the end of either row"""
    u = np.union1d(x, y)
    last = min(x[-1], y[-1]) if len(x) and len(y) else -1
    return int(min(size, np.searchsorted(u, last, side="right")))


def contain_steps(x, y):
    """steps of the containment walk (kernels/sigcontain.hpp): union elements taken until the end of either row, no cap"""
    if not len(x) or not len(y):
        return 0
    return int(np.searchsorted(np.union1d(x, y), min(x[-1], y[-1]), side="right"))


def count_steps(rng, sig, length, sample=20000):
    n = len(sig)
    pairs = n * (n - 1) // 2
    if pairs <= sample:
        idx = [(a, b) for a in range(n) for b in range(a + 1, n)]
    else:
        a = rng.integers(0, n, sample)
        b = rng.integers(0, n, sample)
        idx = [(min(x, y), max(x, y)) for x, y in zip(a.tolist(), b.tolist()) if x != y]
    total = sum(merge_steps(sig[a, :length[a]].astype(np.int64), sig[b, :length[b]].astype(np.int64), sig.shape[1]) for a, b in idx)
    return total / len(idx) * pairs, len(idx) < pairs


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def numpy_top_k(pairs, n, k):
    """rules 2 - 6 of ani_signature_neighbors over the pair rows, minIdentity 0: a dense matrix of keys identityBits << 32 |
    (0xffffffff - neighbour), 0 where there is no pair, the k largest of each row by partition, then sorted"""
    from fastani_amd.api import NEIGHBOR_DT
    a, b = pairs["a"].astype(np.int64), pairs["b"].astype(np.int64)
    ident = pairs["identity"].view(np.uint32).astype(np.uint64) << np.uint64(32)
    key = np.zeros((n, n), dtype=np.uint64)
    key[a, b] = ident | (np.uint64(0xffffffff) - b.astype(np.uint64))
    key[b, a] = ident | (np.uint64(0xffffffff) - a.astype(np.uint64))
    shared = np.zeros((n, n), dtype=np.uint16)
    size = np.zeros((n, n), dtype=np.uint16)
    shared[a, b] = shared[b, a] = pairs["shared"]
    size[a, b] = size[b, a] = pairs["size"]
    kk = min(k, n)
    top = -np.sort(-np.partition(key, n - kk, axis=1)[:, n - kk:].view(np.int64), axis=1)      # (keys are below 2^63: identities are at most 100.0)
    top = top.astype(np.uint64)
    have = top != 0
    nb = np.where(have, np.uint64(0xffffffff) - (top & np.uint64(0xffffffff)), 0).astype(np.int64)
    out = np.zeros((n, k), dtype=NEIGHBOR_DT)
    out["neighbor"] = -1
    rows = np.arange(n)[:, None]
    out["neighbor"][:, :kk] = np.where(have, nb, -1)
    out["shared"][:, :kk] = np.where(have, shared[rows, nb], 0)
    out["size"][:, :kk] = np.where(have, size[rows, nb], 0)
    out["identity"][:, :kk] = (top >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return out, have.sum(axis=1).astype(np.int32)


def neighbors(e, a):
    rng = np.random.default_rng(1)
    for n in (1000, 10000, 65536, 90000):
        if a.only and n != a.only:
            continue
        sig, length = synthetic_signatures(rng, n)
        got = {}
        t = timed(lambda: got.__setitem__("r", e.signature_neighbors(sig, length, 16, a.k)), a.reps)
        nb, count = got["r"]
        line = "neighbors  n=%6d s=%d k=%d: %10.3f ms   %d strips   %d lists full, nearest estimate %.2f .. %.2f" % (
            n, SIZE, a.k, t * 1e3, e.signature_neighbors_strips(), int((count == a.k).sum()), float(nb["identity"][:, 0].min()), float(nb["identity"][:, 0].max()))
        if n <= a.compose_max:
            rows = {}
            tp = timed(lambda: rows.__setitem__("p", e.signature_pairs(sig, length, 16, 1)), a.reps)
            want = {}
            tk = timed(lambda: want.__setitem__("r", numpy_top_k(rows["p"], n, a.k)), a.reps)
            wnb, wcount = want["r"]
            assert np.array_equal(count, wcount) and all(np.array_equal(nb[f], wnb[f]) for f in ("neighbor", "shared", "size"))
            assert np.array_equal(nb["identity"].view(np.uint32), wnb["identity"].view(np.uint32))
            line += "   composition: pairs %.3f ms (%d rows) + numpy top-k %.3f ms = %.3f ms, lists identical" % (tp * 1e3, len(rows["p"]), tk * 1e3, (tp + tk) * 1e3)
        else:
            line += "   composition: not run"
        print(line, flush=True)


def timed_events(fn, reps):
    """1 warm-up + reps calls -> (wall seconds, HIP-event seconds) of each; the events are recorded right before and after the call,
    which returns after its last copy"""
    import torch
    fn()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) / 1e3)
    return wall, dev


def span(ts):
    return "%.3f .. %.3f ms" % (min(ts) * 1e3, max(ts) * 1e3)


def screen(e, a):
    from fastani_amd.api import NEIGHBOR_DT
    rng = np.random.default_rng(1)
    n_ref, shape_env = 10000, "ANI_TEST_SIG_SCREEN_SHAPE"
    ref, ref_len = synthetic_signatures(rng, n_ref)
    qry_all, qry_len_all = synthetic_signatures(rng, 1000)
    qry_all[0], qry_len_all[0] = ref[77], ref_len[77]                  # one query that is a reference
    for n_qry in (1, 16, 1000):
        if a.only and n_qry != a.only:
            continue
        qry, qry_len = qry_all[:n_qry], qry_len_all[:n_qry]
        got, dev_of = {}, {}
        for shape in (None, "square", "thin"):
            os.environ.pop(shape_env, None)
            if shape:
                os.environ[shape_env] = shape
            wall, dev = timed_events(lambda: got.__setitem__(shape, e.signature_screen(ref, ref_len, qry, qry_len, 16, a.k)), a.reps)
            dev_of[shape] = dev
            print("screen     nQry=%5d nRef=%d s=%d k=%d shape %-7s tile %2d x %2d, %d strips: wall %s   HIP events %s"
                  % ((n_qry, n_ref, SIZE, a.k, shape or "default") + e.signature_screen_tile() + (e.signature_screen_strips(), span(wall), span(dev))), flush=True)
        os.environ.pop(shape_env, None)
        for shape in ("square", "thin"):
            assert all(np.array_equal(got[shape][i], got[None][i]) for i in (0, 1)), shape
        # the route without the call: neighbour lists of the query rows over references + queries, cut to the references on the host
        sig, length = np.concatenate([ref, qry]), np.concatenate([ref_len, qry_len])
        old = {}

        def route():
            nb, _ = e.signature_neighbors(sig, length, 16, 1024, rows=(n_ref, n_ref + n_qry))
            out = np.zeros((n_qry, a.k), dtype=NEIGHBOR_DT)
            out["neighbor"] = -1
            count = np.zeros(n_qry, dtype=np.int32)
            for q in range(n_qry):
                keep = nb[q][(nb[q]["neighbor"] >= 0) & (nb[q]["neighbor"] < n_ref)][:a.k]
                out[q, :len(keep)] = keep
                count[q] = len(keep)
            old["r"] = (out, count)

        wall, dev = timed_events(route, a.reps)
        exact = n_qry - 1 + a.k <= 1024                                # (the 1024 entries hold the k references whatever the queries among them)
        same = all(np.array_equal(old["r"][i], got[None][i]) for i in (0, 1))
        assert same or not exact
        print("neighbours nQry=%5d nRef=%d s=%d k=1024 + host cut, %d strips: wall %s   HIP events %s   lists %s   screen / route by HIP events: %.3f .. %.3f"
              % (n_qry, n_ref, SIZE, e.signature_neighbors_strips(), span(wall), span(dev), "identical" if same else "differ (cut too short)",
                 min(dev_of[None]) / max(dev), max(dev_of[None]) / min(dev)), flush=True)


def contain(e, a):
    """ani_signature_screen_contain beside ani_signature_screen: the same signatures, query counts and tile shapes as screen()"""
    rng = np.random.default_rng(1)
    n_ref, shape_env = 10000, "ANI_TEST_SIG_SCREEN_SHAPE"
    ref, ref_len = synthetic_signatures(rng, n_ref)
    qry_all, qry_len_all = synthetic_signatures(rng, 1000)
    qry_all[0], qry_len_all[0] = ref[77], ref_len[77]                  # one query that is a reference
    for n_qry in (1, 16, 1000):
        if a.only and n_qry != a.only:
            continue
        qry, qry_len = qry_all[:n_qry], qry_len_all[:n_qry]
        # the steps of both rules, replayed: every pair up to 20 000 of them, a sample beyond
        pairs = n_qry * n_ref
        if pairs <= 20000:
            idx = [(q, r) for q in range(n_qry) for r in range(n_ref)]
        else:
            idx = list(zip(rng.integers(0, n_qry, 20000).tolist(), rng.integers(0, n_ref, 20000).tolist()))
        rows = [(qry[q, :qry_len[q]].astype(np.int64), ref[r, :ref_len[r]].astype(np.int64)) for q, r in idx]
        steps = {"screen": sum(merge_steps(x, y, SIZE) for x, y in rows) / len(idx) * pairs, "contain": sum(contain_steps(x, y) for x, y in rows) / len(idx) * pairs}
        print("steps      nQry=%5d nRef=%d s=%d (%s): Mash merge %.3e, containment walk %.3e, ratio %.3f"
              % (n_qry, n_ref, SIZE, "exact" if len(idx) == pairs else "sampled", steps["screen"], steps["contain"], steps["contain"] / steps["screen"]), flush=True)
        for shape in (None, "square", "thin"):
            os.environ.pop(shape_env, None)
            if shape:
                os.environ[shape_env] = shape
            per = {}
            for name, fn in (("screen", lambda: e.signature_screen(ref, ref_len, qry, qry_len, 16, a.k)),
                             ("contain", lambda: e.signature_screen_contain(ref, ref_len, qry, qry_len, 16, a.k, a.contain))):
                wall, dev = timed_events(fn, a.reps)
                per[name] = dev
                print("%-10s nQry=%5d nRef=%d s=%d k=%d shape %-7s tile %2d x %2d, %d strips: wall %s   HIP events %s   median %.3f ms   %.3e steps/s"
                      % ((name + (" " + a.contain if name == "contain" else ""), n_qry, n_ref, SIZE, a.k, shape or "default") + e.signature_screen_tile()
                         + (e.signature_screen_strips(), span(wall), span(dev), float(np.median(dev)) * 1e3, steps[name] / float(np.median(dev)))), flush=True)
            ratio = lambda c, s: (c / steps["contain"]) / (s / steps["screen"])
            print("           time per step, contain / screen: %.3f by the medians, %.3f .. %.3f over the spread of both"
                  % (ratio(float(np.median(per["contain"])), float(np.median(per["screen"]))), ratio(min(per["contain"]), max(per["screen"])),
                     ratio(max(per["contain"]), min(per["screen"]))), flush=True)
        os.environ.pop(shape_env, None)


def family_signatures(rng, n, size=SIZE, family=10):
    """n genomes in families of `family`: an ancestor of 1.3 size random 32-bit values, every member loses a share of them drawn from
    0 .. 15 % and gains as many new ones; families are unrelated and share nothing.  In random order, so that the members of a family
    lie in different strips, before and after their representative."""
    sig = np.zeros((n, size), dtype=np.uint32)
    length = np.zeros(n, dtype=np.int32)
    order = rng.permutation(n)
    m = size * 13 // 10
    for f in range(0, n, family):
        anc = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
        for g in order[f:f + family]:
            rate = rng.uniform(0.0, 0.15)
            new = rng.integers(0, 2 ** 32, int(m * rate), dtype=np.uint64).astype(np.uint32)
            v = np.unique(np.concatenate([anc[rng.random(m) >= rate], new]))[:size]
            sig[g, :len(v)] = v
            length[g] = len(v)
    return sig, length


def cluster(e, a):
    from fastani_amd.api import CGI_DT
    rng = np.random.default_rng(1)
    for n in (10000, 90000):
        if a.only and n != a.only:
            continue
        sig, length = family_signatures(rng, n)
        got = {}
        wall, dev = timed_events(lambda: got.__setitem__("r", e.signature_cluster(sig, length, 16, a.cluster)), a.reps)
        rep, link = got["r"]
        strips, reps, cells, steps = e.signature_cluster_stats()
        own = rep == np.arange(n)
        assert reps == int(own.sum())
        print("cluster    n=%6d s=%d T=%g: HIP events %s median %.3f ms   wall %s   %d strips, %d representatives, %.3e cells merged (n^2/2 = %.3e), %d resolve steps"
              "   %d members joined a later representative, estimate to the representative %.2f .. %.2f"
              % (n, SIZE, a.cluster, span(dev), float(np.median(dev)) * 1e3, span(wall), strips, reps, cells, n * n / 2, steps, int((rep > np.arange(n)).sum()),
                 float(link["identity"][~own].min()) if (~own).any() else 0.0, float(link["identity"][~own].max()) if (~own).any() else 0.0), flush=True)
        if n > a.compose_max:
            print("composition n=%6d: not run (ani_signature_pairs takes at most 65 536 genomes)" % n, flush=True)
            continue
        old = {}

        def composition():
            pairs = e.signature_pairs(sig, length, 16, 1)
            rows = np.zeros(len(pairs), dtype=CGI_DT)
            rows["refGenomeId"], rows["qryGenomeId"], rows["identity"] = pairs["a"], pairs["b"], pairs["identity"]
            old["r"], old["rows"] = e.cluster_greedy(rows, n, a.cluster), len(pairs)

        cwall, cdev = timed_events(composition, a.reps)
        wrep, wident = old["r"]
        same = np.array_equal(rep, wrep) and np.array_equal(link["identity"][~own].view(np.uint32), wident[~own].view(np.uint32))
        assert same
        print("composition n=%6d s=%d T=%g: HIP events %s median %.3f ms   wall %s   %d pair rows   result identical   call / composition by HIP events: %.3f .. %.3f"
              % (n, SIZE, a.cluster, span(cdev), float(np.median(cdev)) * 1e3, span(cwall), old["rows"], min(dev) / max(cdev), max(dev) / min(cdev)), flush=True)


def cluster_contain(e, a):
    """ani_signature_cluster_contain beside itself without the triangular block and beside ani_signature_cluster: the genomes of
    cluster(), the three calls in turns so that a drift of the machine meets all of them"""
    rng = np.random.default_rng(1)
    tri_env = "ANI_TEST_SIG_CLUSTER_TRI"
    calls = (("contain", None, lambda sig, length: e.signature_cluster_contain(sig, length, 16, a.cluster, a.contain)),
             ("contain, full blocks", "0", lambda sig, length: e.signature_cluster_contain(sig, length, 16, a.cluster, a.contain)),
             ("mash", None, lambda sig, length: e.signature_cluster(sig, length, 16, a.cluster)))
    for n in (10000, 90000):
        if a.only and n != a.only:
            continue
        sig, length = family_signatures(rng, n)
        wall, dev, got, stats = ({name: [] for name, _, _ in calls} for _ in range(4))
        for turn in range(a.reps + 1):                                 # (the first turn warms up)
            for name, tri, fn in calls:
                os.environ.pop(tri_env, None)
                if tri is not None:
                    os.environ[tri_env] = tri
                w, d = timed_once(lambda: got.__setitem__(name, fn(sig, length)))
                stats[name] = e.signature_cluster_stats()
                if turn:
                    wall[name] += w
                    dev[name] += d
        os.environ.pop(tri_env, None)
        for i in (0, 1):
            assert np.array_equal(got["contain"][i], got["contain, full blocks"][i])
        for name, _, _ in calls:
            rep, link = got[name]
            own = rep == np.arange(n)
            strips, reps, cells, steps = stats[name]
            assert reps == int(own.sum())
            print("cluster    n=%6d s=%d T=%g %-20s: HIP events %s median %.3f ms   wall %s median %.3f ms   %d strips, %d representatives, %.3e cells walked, "
                  "%d resolve steps   %d members joined a later representative"
                  % (n, SIZE, a.cluster, name, span(dev[name]), float(np.median(dev[name])) * 1e3, span(wall[name]), float(np.median(wall[name])) * 1e3, strips, reps,
                     cells, steps, int((rep > np.arange(n)).sum())), flush=True)
        m = {name: float(np.median(dev[name])) for name, _, _ in calls}
        print("           n=%6d: results of the two containment calls identical; by the medians of the HIP events, contain / contain with full blocks %.3f, "
              "contain / mash %.3f" % (n, m["contain"] / m["contain, full blocks"], m["contain"] / m["mash"]), flush=True)


def timed_once(fn):
    """one call of timed_events without its warm-up"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    wall = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return [wall], [e0.elapsed_time(e1) / 1e3]


def graph(e, a):
    rng = np.random.default_rng(1)
    estimate = "contain" if a.contain else "mash"
    low = np.float32(a.graph).view(np.uint32)
    for n in (10000, 90000):
        if a.only and n != a.only:
            continue
        sig, length = family_signatures(rng, n)
        got = {}
        wall, dev = timed_events(lambda: got.__setitem__("r", e.signature_graph(sig, length, 16, a.graph, 1, estimate)), a.reps)
        print("graph      n=%6d s=%d T=%g %s: HIP events %s median %.3f ms   wall %s median %.3f ms   %d strips, %d kept pairs"
              % (n, SIZE, a.graph, estimate, span(dev), float(np.median(dev)) * 1e3, span(wall), float(np.median(wall)) * 1e3, e.signature_graph_strips(), len(got["r"])),
              flush=True)
        if estimate != "mash" or n > a.compose_max:
            print("composition n=%6d: not run (%s)" % (n, "ani_signature_pairs knows the Mash estimate only" if estimate != "mash"
                                                      else "ani_signature_pairs takes at most 65 536 genomes"), flush=True)
            continue
        old = {}

        def composition():
            pairs = e.signature_pairs(sig, length, 16, 1)
            old["r"], old["rows"] = pairs[pairs["identity"].view(np.uint32) >= low], len(pairs)

        cwall, cdev = timed_events(composition, a.reps)
        assert np.array_equal(got["r"], old["r"])
        print("composition n=%6d s=%d T=%g: HIP events %s median %.3f ms   wall %s median %.3f ms   %d pair rows   records identical   call / composition by the wall clock: "
              "%.3f .. %.3f" % (n, SIZE, a.graph, span(cdev), float(np.median(cdev)) * 1e3, span(cwall), float(np.median(cwall)) * 1e3, old["rows"],
                                min(wall) / max(cwall), max(wall) / min(cwall)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-shared", type=int, default=SIZE + 1)
    ap.add_argument("--skip-signatures", action="store_true")
    ap.add_argument("--neighbors", action="store_true")
    ap.add_argument("--screen", action="store_true")
    ap.add_argument("--contain", choices=("query", "reference", "max"), default=None)
    ap.add_argument("--cluster", type=float, default=0.0)
    ap.add_argument("--graph", type=float, default=0.0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--compose-max", type=int, default=10000)
    a = ap.parse_args()
    if a.contain and not a.screen and not a.graph and not a.cluster:
        ap.error("--contain needs --screen, --graph or --cluster")
    if a.graph and a.contain not in (None, "max"):
        ap.error("--graph takes --contain max only")
    if a.cluster and a.contain not in (None, "max"):
        ap.error("--cluster takes --contain max only")
    if a.neighbors or a.screen or a.cluster or a.graph:
        import fastani_amd
        (graph if a.graph else cluster_contain if a.cluster and a.contain else cluster if a.cluster else neighbors if a.neighbors else contain if a.contain else screen)(fastani_amd.engine(0), a)
        return
    import torch
    import fastani_amd
    from fastani_amd.api import DeviceGenomes, Sketch
    e = fastani_amd.engine(0)
    rng = np.random.default_rng(1)
    for n in (1000, 10000, 65536):
        if a.only and n != a.only:
            continue
        sig, length = synthetic_signatures(rng, n)
        steps, sampled = count_steps(rng, sig, length)
        out = {}
        t = timed(lambda: out.__setitem__("rows", len(e.signature_pairs(sig, length, 16, a.min_shared))), a.reps)
        print("pairs      n=%6d s=%d: %9.3f ms   %.3e merge steps (%s)   %.3e steps/s   %d rows at minShared %d"
              % (n, SIZE, t * 1e3, steps, "sampled" if sampled else "exact", steps / t, out["rows"], a.min_shared), flush=True)
        if a.skip_signatures:
            continue
        L = GENOME_LEN[n]
        words = (L + 15) // 16
        buf = torch.empty(n * words, dtype=torch.int32, device="cuda:0")
        e.synth_packed(5, 0, n, L, buf.data_ptr())
        torch.cuda.synchronize()
        sk = Sketch(e, e.params(16, 3000), DeviceGenomes(buf.data_ptr(), n, L))
        got = {}
        t = timed(lambda: got.__setitem__("len", sk.signatures(SIZE)[1]), a.reps)
        print("signatures n=%6d s=%d: %9.3f ms   %d minimizers of %d-base genomes, %d full signatures"
              % (n, SIZE, t * 1e3, sk.stats()["minimizers"], L, int((got["len"] == SIZE).sum())), flush=True)
        sk.close()
        del buf


if __name__ == "__main__":
    main()
