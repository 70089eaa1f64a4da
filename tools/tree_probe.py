"""Timings of ani_tree_average (average-linkage tree), with --method nj of ani_tree_nj (neighbour joining,
section 2.13), with --method single of ani_tree_single (single linkage / minimum spanning tree, section 2.15) and with --method
single-sketch of ani_tree_single_sketch (the same with the sketch fill, streamed, section 2.16) on synthetic row sets, on the GPU.  The call returns after its last device-to-host copy, so the wall clock around it
includes the upload, the matrix, every merge launch and the read-back.

    python tools/tree_probe.py                 the row sets below, 1 warm-up + 3 timed calls each (median reported)
    python tools/tree_probe.py --only hub      only the row sets whose name starts with that (e.g. under rocprofv3)
    python tools/tree_probe.py --method nj     ani_tree_nj on the same row sets, with the bytes its scans read by its own model
                                               (nj_scan_bytes) and the rate that makes of the median
    python tools/tree_probe.py --method single ani_tree_single on the same row sets and on "species 150000" (above the dense trees'
                                               ceiling), with its spanning-forest rounds, and ani_cluster_greedy at 95 on the same rows
                                               as the yardstick: both calls upload, sort and fold the rows, so the difference is
                                               what the forest stage costs
    python tools/tree_probe.py --method single-sketch
                                               ani_tree_single_sketch (section 2.16) on species rows plus signatures of 1000 values for
                                               1 000, 10 000, 65 536 and 90 000 genomes: wall clock, strips, rounds and the edges each
                                               strip kept; beside it ani_signature_pairs + the fill rule + ani_tree_single on the same
                                               input, up to --compose-max genomes (default 10 000: the composition brings every pair
                                               that shares a value to the host, 1.5 * 10^9 rows at 65 536), and the two results compared
    python tools/tree_probe.py --support 100   ani_tree_support_bootstrap (section 2.29) per method on species 1000 and species 10000 at
                                               that many replicates, beside B times the plain call, one upload of the rows' bytes and
                                               ani_tree_support alone; --support-budget S leaves out what B plain calls would take
                                               longer than (default 60 s)
    python tools/tree_probe.py --reps 1        timed calls per row set (default 3)
    python tools/tree_probe.py --cli 1000      in addition: fastANI --ql L --rl L --tree on that many 5 Mbp genomes, the
                                               ANI_CLI_TRACE marks of the run ("rows ordered" -> "tree written" is the tree's share)

Row sets (identities from cluster_probe.species_rows: species of 50, ANI >= 95 inside, 78-95 across, both directions of a pair):
    species 1000     10^5 rows over 1 000 genomes
    species 10000    10^6 rows over 10 000 genomes
    species 65536    4 * 10^6 rows over 65 536 genomes (the largest tree: a 17 GB matrix)
    path 2000        an ordered path of 2 000 genomes, every other pair missing
    hub 2000         genome 0 close to all 1 999 others, which are far from each other: the first merge rescans every row
    species 150000   10^7 rows over 150 000 genomes (--method single only)
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def path_rows(m):
    from fastani_amd.api import CGI_DT
    rows = np.zeros(m - 1, dtype=CGI_DT)
    rows["qryGenomeId"] = np.arange(1, m, dtype=np.int32)
    rows["refGenomeId"] = np.arange(0, m - 1, dtype=np.int32)
    rows["identity"] = 97.0 - (np.arange(m - 1) % 7).astype(np.float32) * np.float32(0.5)
    return rows


def hub_rows(m):
    from fastani_amd.api import CGI_DT
    rows = np.zeros(2 * (m - 1) - 1, dtype=CGI_DT)
    rows["qryGenomeId"][:m - 1], rows["refGenomeId"][:m - 1], rows["identity"][:m - 1] = 0, np.arange(1, m), 99.0
    rows["qryGenomeId"][m - 1:], rows["refGenomeId"][m - 1:], rows["identity"][m - 1:] = np.arange(1, m - 1), np.arange(2, m), 80.0
    return rows


def nj_scan_bytes(n):
    """what the scans of one ani_tree_nj call read, by the host loop of tree_nj (engine_graph.hip): record s scans the tiles of 256
    columns x 16 or 64 rows that reach above the diagonal of the current matrix, 4 bytes per cell, and the matrix is compacted to the
    active positions whenever an eighth of its positions is retired -> (bytes, cells of the active upper triangles: the n^3 / 6)"""
    cur, total, ideal = n, 0, 0
    for s in range(n - 1):
        rows_per_tile = 16 if cur <= 4096 else 64
        r0 = np.arange(0, cur, rows_per_tile)
        r1 = np.minimum(r0 + rows_per_tile, cur)
        first = np.where(r0 >= 255, (r0 - 255) // 256 + 1, 0)       # the first tile column with c0 + 255 > r0
        ld = (cur + 63) // 64 * 64
        cols = np.maximum(ld - first * 256, 0)
        total += int(((r1 - r0) * cols).sum()) * 4
        m = n - s
        ideal += m * (m - 1) // 2
        if s + 2 < n and cur > 64 and 8 * (m - 1) <= 7 * cur:
            cur = m - 1
    return total, ideal


def time_call(e, rows, n, reps=3, method="average"):
    children = np.empty(2 * (n - 1), dtype=np.int32)
    height = np.empty(2 * (n - 1), dtype=np.float32)
    fn = e.lib.ani_tree_nj if method == "nj" else e.lib.ani_tree_average

    def call():
        rc = fn(e.h, rows.ctypes.data, len(rows), n, ctypes.c_float(0.0), children.ctypes.data, height.ctypes.data)
        assert rc == 0, rc
    call()                                                         # warm-up: code objects, pool segments, page-locked staging
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    if method == "nj":
        assert sorted(children.tolist()) == list(range(2 * n - 2))
        return ms, float(height.sum())
    assert (np.diff(height[:n - 1]) >= 0).all()
    return ms, float(height[n - 2])


def time_single(e, rows, n, reps=3):
    """-> (ms of ani_tree_single, rounds, forest edges, ms of ani_cluster_greedy at 95 on the same rows)"""
    children = np.empty(2 * (n - 1), dtype=np.int32)
    height = np.empty(n - 1, dtype=np.float32)
    edges = np.empty(2 * (n - 1), dtype=np.int32)
    rep = np.empty(n, dtype=np.int32)
    ident = np.empty(n, dtype=np.float32)

    def single():
        rc = e.lib.ani_tree_single(e.h, rows.ctypes.data, len(rows), n, ctypes.c_float(0.0), children.ctypes.data, height.ctypes.data, edges.ctypes.data)
        assert rc == 0, rc

    def greedy():
        rc = e.lib.ani_cluster_greedy(e.h, rows.ctypes.data, len(rows), n, ctypes.c_float(95.0), rep.ctypes.data, ident.ctypes.data)
        assert rc == 0, rc
    out = []
    for call in (single, greedy):
        call()                                                     # warm-up: code objects, pool segments, page-locked staging
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        out.append(ms)
    single()                                                       # (the rounds are those of the context's last ani_tree_single call)
    assert (np.diff(height) >= 0).all()
    return out[0], e.tree_single_rounds(), int((height < 1.0).sum()), out[1]


def species_signatures(rng, n, size=1000, per_species=50):
    """signatures of `size` values below size / 5e6 * 2^32, where the bottom values of a 5 Mbp genome lie: unrelated genomes share about
    one value by chance; a genome keeps 60 - 97 % of its species' values"""
    top = int(size / 5e6 * 2 ** 32)
    sig = np.empty((n, size), dtype=np.uint32)
    for s0 in range(0, n, per_species):
        m = min(per_species, n - s0)
        base = rng.integers(0, top, size, dtype=np.uint32)
        own = rng.integers(0, top, (m, size), dtype=np.uint32)
        keep = rng.random((m, size)) < rng.uniform(0.6, 0.97, (m, 1))
        sig[s0:s0 + m] = np.where(keep, base[None, :], own)
    sig.sort(axis=1)
    length = np.full(n, size, dtype=np.int32)
    for g in np.nonzero((np.diff(sig.astype(np.int64), axis=1) <= 0).any(axis=1))[0]:      # a repeated value: the distinct ones, a shorter row
        u = np.unique(sig[g])
        sig[g] = 0
        sig[g, :len(u)] = u
        length[g] = len(u)
    return sig, length


def time_single_sketch(e, rows, n, sig, length, reps=3, compose=True):
    from fastani_amd.api import CGI_DT

    def streamed():
        return e.tree_single_sketch(rows, n, sig, length, 16, 1, 0.0, return_edges=True, return_source=True)

    def composed():
        pairs = e.signature_pairs(sig, length, 16, 1)
        q, r = rows["qryGenomeId"].astype(np.int64), rows["refGenomeId"].astype(np.int64)
        have = np.unique(np.minimum(q, r)[q != r] * n + np.maximum(q, r)[q != r])
        fill = pairs[(pairs["identity"] > 0) & ~np.isin(pairs["a"].astype(np.int64) * n + pairs["b"], have)]
        extra = np.zeros(len(fill), dtype=CGI_DT)
        extra["qryGenomeId"], extra["refGenomeId"], extra["identity"] = fill["a"], fill["b"], fill["identity"]
        return e.tree_single(np.concatenate([rows, extra]), n, 0.0, return_edges=True) + (len(pairs),)
    out = []
    for call in (streamed, composed) if compose else (streamed,):
        result = call()                                            # warm-up: code objects, pool segments, page-locked staging
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            result = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        out.append((ms, result))
        if call is streamed:
            strips, rounds = e.tree_single_sketch_strips(), e.tree_single_rounds()
    (ms, (z, edges, source)) = out[0]
    line = "ani_tree_single_sketch %s ms (median %.1f)   %d strips, %d rounds, edges kept per strip %s   merges from rows / sketch / joins %s" % (
        " ".join("%.1f" % x for x in ms), float(np.median(ms)), len(strips), rounds, " ".join(str(int(x)) for x in strips),
        " / ".join(str(int(x)) for x in np.bincount(source, minlength=3)))
    if compose:
        (cms, (cz, cedges, npairs)) = out[1]
        same = np.array_equal(z, cz) and np.array_equal(edges, cedges)
        line += "   signature_pairs + fill + tree_single %s ms (median %.1f, %d pair rows)   %s" % (
            " ".join("%.1f" % x for x in cms), float(np.median(cms)), npairs, "identical" if same else "DIFFERENT")
    return line


def support_run(e, rng, replicates, only, reps, budget_s):
    """--support B: ani_tree_support_bootstrap per method at 1000 and 10 000 genomes beside B times the plain tree call and the support
    count alone, with the time one plain host-to-device copy of the rows' bytes takes — an estimate of the share B uploads of the same
    ids have in the composed call; the engine's own upload goes through page-locked staging and feeds a sort, and is not timed apart.  The
    replicate identities are the rows' own moved by up to 0.5.  A size whose B plain calls would pass --support-budget seconds is left out
    and said so."""
    import torch
    from cluster_probe import species_rows
    from fastani_amd.api import tree_support
    for n, n_rows in ((1000, 10 ** 5), (10000, 10 ** 6)):
        if not ("species %d" % n).startswith(only):
            continue
        rows = species_rows(rng, n, n_rows)
        rep = np.clip(rows["identity"][:, None] + rng.uniform(-0.5, 0.5, (len(rows), replicates)).astype(np.float32), 1.0, 100.0).astype(np.float32)
        raw = torch.from_numpy(rows.view(np.uint8).copy())
        up = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            raw.to("cuda:0")
            torch.cuda.synchronize()
            up.append((time.perf_counter() - t0) * 1e3)
        up_ms = float(np.median(up[1:]))
        for method in ("average", "nj", "single"):
            call = {"average": e.tree_average, "nj": e.tree_nj, "single": e.tree_single}[method]
            main = call(rows, n)
            children = (main[0] if method == "nj" else main[:, 0:2]).astype(np.int32)
            plain = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call(rows, n)
                plain.append((time.perf_counter() - t0) * 1e3)
            pm = float(np.median(plain))
            head = "species %-6d rows %9d genomes %6d %-7s B %d   plain call %.2f ms, B of them %.1f ms; one plain host-to-device copy of the rows' bytes (%.1f MB; an estimate of the engine's upload, which also stages and sorts) %.3f ms, B of them %.1f ms" % (
                n, len(rows), n, method, replicates, pm, pm * replicates, rows.nbytes / 1e6, up_ms, up_ms * replicates)
            if pm * replicates / 1e3 > budget_s:
                print(head + "   composed call NOT RUN: past the budget of %g s" % budget_s, flush=True)
                continue
            ms = []
            for _ in range(max(1, min(reps, int(budget_s * 1e3 / (pm * replicates))))):
                t0 = time.perf_counter()
                support = e.tree_support_bootstrap(method, rows, n, rep, children)
                ms.append((time.perf_counter() - t0) * 1e3)
            med = float(np.median(ms))
            same = [children] * replicates
            t0 = time.perf_counter()
            tree_support(children, same, method == "nj", lib=e.lib)
            count_ms = (time.perf_counter() - t0) * 1e3
            print(head + "   ani_tree_support_bootstrap %s ms (median %.1f = %.2f x B plain calls; the copies, by that estimate, %.1f %% of it)   ani_tree_support alone over B trees %.2f ms"
                  "   support min %d median %d max %d" % (" ".join("%.1f" % x for x in ms), med, med / (pm * replicates), 100.0 * up_ms * replicates / med, count_ms,
                                                           int(support.min()), int(np.median(support)), int(support.max())), flush=True)
        del rows, rep
    return 0


def cli_run(n):
    import bench
    import orc
    td = tempfile.mkdtemp(prefix="ani_tree_", dir="/tmp")
    t0 = time.time()
    paths = bench.write_fasta_set(orc, 20260925, list(range(n)), 5000000, td, 16)
    print("wrote %d genomes in %.1f s" % (n, time.time() - t0), flush=True)
    lst = os.path.join(td, "all.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    cli = os.path.join(ROOT, "fastani_amd", "fastANI")
    for rep in range(2):
        out = os.path.join(td, "out.txt")
        r = subprocess.run([cli, "--ql", lst, "--rl", lst, "-t", "16", "--tree", "-o", out], capture_output=True,
                           env=dict(os.environ, ANI_CLI_TRACE="1"), timeout=600)
        print("run %d: exit %d" % (rep, r.returncode))
        for ln in r.stderr.decode(errors="replace").splitlines():
            if "[fastANI trace]" in ln:
                print("  " + ln)
        if r.returncode != 0:
            print(r.stderr.decode(errors="replace")[-2000:])
            return 1
        print("  .newick %d bytes, %d rows in %s" % (os.path.getsize(out + ".newick"), sum(1 for _ in open(out)), out))
    return 0


def main():
    import fastani_amd
    from cluster_probe import species_rows
    e = fastani_amd.engine(0)
    rng = np.random.default_rng(7)
    sets = [("species 1000", lambda: species_rows(rng, 1000, 10 ** 5), 1000),
            ("species 10000", lambda: species_rows(rng, 10000, 10 ** 6), 10000),
            ("species 65536", lambda: species_rows(rng, 65536, 4 * 10 ** 6), 65536),
            ("path 2000", lambda: path_rows(2000), 2000),
            ("hub 2000", lambda: hub_rows(2000), 2000)]
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    method = sys.argv[sys.argv.index("--method") + 1] if "--method" in sys.argv else "average"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    assert method in ("average", "nj", "single", "single-sketch"), method
    if "--support" in sys.argv:
        budget = float(sys.argv[sys.argv.index("--support-budget") + 1]) if "--support-budget" in sys.argv else 60.0
        return support_run(e, rng, int(sys.argv[sys.argv.index("--support") + 1]), only, reps, budget)
    if method == "single-sketch":
        compose_max = int(sys.argv[sys.argv.index("--compose-max") + 1]) if "--compose-max" in sys.argv else 10000
        for n in (1000, 10000, 65536, 90000):
            if not ("species %d" % n).startswith(only):
                continue
            rows = species_rows(rng, n, 100 * n)
            sig, length = species_signatures(rng, n)
            print("species %-6d rows %9d genomes %6d size 1000   %s" % (n, len(rows), n, time_single_sketch(e, rows, n, sig, length, reps, n <= compose_max)),
                  flush=True)
            del rows, sig
        return 0
    if method == "single":
        sets.append(("species 150000", lambda: species_rows(rng, 150000, 10 ** 7), 150000))
    for name, make, n in sets:
        if not name.startswith(only):
            continue
        rows = make()
        if method == "single":
            ms, rounds, forest, greedy_ms = time_single(e, rows, n, reps)
            med, gmed = float(np.median(ms)), float(np.median(greedy_ms))
            print("%-14s rows %9d genomes %6d   ani_tree_single %s ms (median %.2f)   %d rounds, %d forest edges   ani_cluster_greedy(95) %s ms "
                  "(median %.2f)   difference %.2f ms"
                  % (name, len(rows), n, " ".join("%.2f" % x for x in ms), med, rounds, forest, " ".join("%.2f" % x for x in greedy_ms), gmed, med - gmed),
                  flush=True)
            del rows
            continue
        ms, top = time_call(e, rows, n, reps, method)
        if method == "nj":
            med = float(np.median(ms))
            nbytes, ideal = nj_scan_bytes(n)
            print("%-14s rows %9d genomes %6d   ani_tree_nj %s ms (median %.1f, %.2f us per join)   scans read %.3f GB = %.2f x the %.3g "
                  "active cells -> %.2f TB/s   tree length %.4f"
                  % (name, len(rows), n, " ".join("%.1f" % x for x in ms), med, med * 1e3 / (n - 1), nbytes / 1e9, nbytes / 4 / ideal, ideal,
                     nbytes / med / 1e9, top), flush=True)
            del rows
            continue
        print("%-14s rows %9d genomes %6d   ani_tree_average %s ms (median %.1f, %.2f us per merge)   root height %.4f"
              % (name, len(rows), n, " ".join("%.1f" % x for x in ms), float(np.median(ms)), float(np.median(ms)) * 1e3 / (n - 1), top), flush=True)
        del rows
    if "--cli" in sys.argv:
        return cli_run(int(sys.argv[sys.argv.index("--cli") + 1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
