"""Timings of ani_tree_average (average-linkage tree) on synthetic row sets, on the GPU.  The call returns
after its last device-to-host copy, so the wall clock around it includes the upload, the matrix, every merge launch and the read-back.

    python tools/tree_probe.py                 the row sets below, 1 warm-up + 3 timed calls each (median reported)
    python tools/tree_probe.py --only hub      only the row sets whose name starts with that (e.g. under rocprofv3)
    python tools/tree_probe.py --cli 1000      in addition: fastANI --ql L --rl L --tree on that many 5 Mbp genomes, the
                                               ANI_CLI_TRACE marks of the run ("rows ordered" -> "tree written" is the tree's share)

Row sets (identities from cluster_probe.species_rows: species of 50, ANI >= 95 inside, 78-95 across, both directions of a pair):
    species 1000     10^5 rows over 1 000 genomes
    species 10000    10^6 rows over 10 000 genomes
    species 65536    4 * 10^6 rows over 65 536 genomes (the largest tree: a 17 GB matrix)
    path 2000        an ordered path of 2 000 genomes, every other pair missing
    hub 2000         genome 0 close to all 1 999 others, which are far from each other: the first merge rescans every row
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


def time_call(e, rows, n, reps=3):
    children = np.empty(2 * (n - 1), dtype=np.int32)
    height = np.empty(n - 1, dtype=np.float32)

    def call():
        rc = e.lib.ani_tree_average(e.h, rows.ctypes.data, len(rows), n, ctypes.c_float(0.0), children.ctypes.data, height.ctypes.data)
        assert rc == 0, rc
    call()                                                         # warm-up: code objects, pool segments, page-locked staging
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert (np.diff(height) >= 0).all()
    return ms, float(height[-1])


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
    for name, make, n in sets:
        if not name.startswith(only):
            continue
        rows = make()
        ms, top = time_call(e, rows, n)
        print("%-14s rows %9d genomes %6d   ani_tree_average %s ms (median %.1f, %.2f us per merge)   root height %.4f"
              % (name, len(rows), n, " ".join("%.1f" % x for x in ms), float(np.median(ms)), float(np.median(ms)) * 1e3 / (n - 1), top), flush=True)
        del rows
    if "--cli" in sys.argv:
        return cli_run(int(sys.argv[sys.argv.index("--cli") + 1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
