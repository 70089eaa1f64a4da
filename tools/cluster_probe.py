"""Timings of ani_cluster_greedy (greedy species clustering) on synthetic row sets, on the GPU.  The call
returns after its last device-to-host copy, so the wall clock around it includes every kernel and the upload.

    python tools/cluster_probe.py                 the four row sets below, 1 warm-up + 3 timed calls each
    python tools/cluster_probe.py --only path     only the row sets whose name starts with that (e.g. under rocprofv3)
    python tools/cluster_probe.py --cli 1000      in addition: fastANI --ql L --rl L --cluster 95 on that many 5 Mbp genomes, the
                                                  ANI_CLI_TRACE marks of the run

Row sets:
    random 1e6      10^6 rows over 10 000 genomes (species of 50: ANI >= 95 inside, < 95 across), both directions of most pairs
    all-vs-all      7.8 * 10^7 rows, the row count of a 10 000 x 10 000 run, the same species structure
    clique 3000     every ordered pair of 3 000 genomes above the threshold (9 * 10^6 rows; lower lists of up to 2 999 neighbours)
    path 1e5        an ordered path of 10^5 genomes (the most rounds: one decision per vertex in sequence)
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def species_rows(rng, n_genomes, n_rows, species=50):
    from fastani_amd.api import CGI_DT
    half = n_rows // 2
    q = rng.integers(0, n_genomes, half, dtype=np.int32)
    # half of the pairs inside a species, the rest anywhere
    same = rng.random(half) < 0.5
    r = np.where(same, q // species * species + rng.integers(0, species, half, dtype=np.int32), rng.integers(0, n_genomes, half, dtype=np.int32))
    r = np.minimum(r, n_genomes - 1).astype(np.int32)
    inside = q // species == r // species
    x = np.where(inside, 95.0 + 5.0 * rng.random(half, dtype=np.float32), 78.0 + 16.9 * rng.random(half, dtype=np.float32)).astype(np.float32)
    rows = np.zeros(2 * half, dtype=CGI_DT)
    rows["qryGenomeId"][:half], rows["refGenomeId"][:half], rows["identity"][:half] = q, r, x
    rows["qryGenomeId"][half:], rows["refGenomeId"][half:] = r, q                       # the other direction, a slightly different value
    rows["identity"][half:] = np.minimum(x + np.float32(0.25) * rng.random(half, dtype=np.float32), np.float32(100))
    return rows


def clique_rows(m):
    from fastani_amd.api import CGI_DT
    a, b = np.meshgrid(np.arange(m, dtype=np.int32), np.arange(m, dtype=np.int32), indexing="ij")
    keep = a != b
    rows = np.zeros(int(keep.sum()), dtype=CGI_DT)
    rows["qryGenomeId"], rows["refGenomeId"] = a[keep], b[keep]
    rows["identity"] = 96.0 + ((a[keep] * 7 + b[keep] * 13) % 32).astype(np.float32) * np.float32(0.125)
    return rows


def path_rows(m):
    from fastani_amd.api import CGI_DT
    rows = np.zeros(m - 1, dtype=CGI_DT)
    rows["qryGenomeId"] = np.arange(1, m, dtype=np.int32)
    rows["refGenomeId"] = np.arange(0, m - 1, dtype=np.int32)
    rows["identity"] = 97.0
    return rows


def time_call(e, rows, n, t, reps=3):
    e.cluster_greedy(rows, n, t)                                   # warm-up: code objects, pool segments, page-locked staging
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rep, _ = e.cluster_greedy(rows, n, t)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, int((rep == np.arange(n)).sum())


def cli_run(n):
    import bench
    import orc
    td = tempfile.mkdtemp(prefix="ani_cluster_", dir="/tmp")
    t0 = time.time()
    paths = bench.write_fasta_set(orc, 20260925, list(range(n)), 5000000, td, 16)
    print("wrote %d genomes in %.1f s" % (n, time.time() - t0), flush=True)
    lst = os.path.join(td, "all.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    cli = os.path.join(ROOT, "fastani_amd", "fastANI")
    for rep in range(2):
        out = os.path.join(td, "out.txt")
        r = subprocess.run([cli, "--ql", lst, "--rl", lst, "-t", "16", "--cluster", "95", "-o", out], capture_output=True,
                           env=dict(os.environ, ANI_CLI_TRACE="1"), timeout=600)
        print("run %d: exit %d" % (rep, r.returncode))
        for ln in r.stderr.decode(errors="replace").splitlines():
            if "[fastANI trace]" in ln:
                print("  " + ln)
        if r.returncode != 0:
            print(r.stderr.decode(errors="replace")[-2000:])
            return 1
        lines = open(out + ".clusters").read().splitlines()
        print("  %d genomes, %d clusters, %d rows in %s" % (len(lines), sum(1 for l in lines if l.endswith("\tNA")), sum(1 for _ in open(out)), out))
    return 0


def main():
    import fastani_amd
    e = fastani_amd.engine(0)
    rng = np.random.default_rng(7)
    sets = [("random 1e6", lambda: species_rows(rng, 10000, 10 ** 6), 10000),
            ("all-vs-all 7.8e7", lambda: species_rows(rng, 10000, 78000000), 10000),
            ("clique 3000", lambda: clique_rows(3000), 3000),
            ("path 1e5", lambda: path_rows(100000), 100000)]
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    for name, make, n in sets:
        if not name.startswith(only):
            continue
        t0 = time.time()
        rows = make()
        gen = time.time() - t0
        ms, nrep = time_call(e, rows, n, 95.0)
        print("%-18s rows %10d genomes %6d representatives %6d   ani_cluster_greedy %s ms (median %.1f)   [rows made in %.1f s]"
              % (name, len(rows), n, nrep, " ".join("%.1f" % x for x in ms), float(np.median(ms)), gen), flush=True)
        del rows
    if "--cli" in sys.argv:
        return cli_run(int(sys.argv[sys.argv.index("--cli") + 1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
