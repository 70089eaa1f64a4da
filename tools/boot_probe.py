"""Cost of the bootstrap replicate records on the GPU: ani_map_cgi_batch of synthetic genomes against
themselves with the mode off and on, same process, same sketch, same inputs, the two taken in turns (off, on, off, on, ...) so that a
drift of the machine meets both; 1 warm-up turn + --reps timed turns, medians reported.

    python tools/boot_probe.py                            200 genomes of 1 Mbp in ONE cluster (a species-dense set: every pair has a row)
    python tools/boot_probe.py --genomes 1000 --genome-len 5000000 --cluster-size 20    the benchmark's set
    python tools/boot_probe.py --replicates 1000 --min-ani 95 --min-fragments 50       more replicates, a gate

Per state: the call by the wall clock and by HIP events around it (it returns after its last copy), and the reducer's own HIP-event
timer (ani_counters_t.msReduce: the bin table's memset, k_oneway_bins, k_pair_reduce and, with the mode on, k_ci_flags, the scans,
k_ci_list, k_boot_records and the copies of the records and the sums to the host).  The new work's share is the difference of the
msReduce medians.  Also: the number of records, the bytes to the host, the pairs that skip the draws (one distinct value) and the draws
(replicates x cells of the others).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    wall = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return wall, e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=200)
    ap.add_argument("--genome-len", type=int, default=1000000)
    ap.add_argument("--cluster-size", type=int, default=0, help="related genomes per cluster (0 = all of them in one)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--boot-seed", type=int, default=1)
    ap.add_argument("--min-ani", type=float, default=0.0)
    ap.add_argument("--min-fragments", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260925)
    a = ap.parse_args()
    import torch
    import fastani_amd
    from fastani_amd.api import DeviceGenomes, Sketch
    e = fastani_amd.engine(0)
    n, L = a.genomes, a.genome_len
    p = e.params(16, 3000)
    buf = torch.empty(n * ((L + 15) // 16), dtype=torch.int32, device="cuda:0")
    e.synth_packed(a.seed, 0, n, L, buf.data_ptr(), variant=0, cluster_size=a.cluster_size or n)
    torch.cuda.synchronize()
    genomes = DeviceGenomes(buf.data_ptr(), n, L)
    sk = Sketch(e, p, genomes)
    print("boot_probe: %d genomes of %d bases, clusters of %d; %d bins of %d bases, %d index chunk(s); %d replicates, seed %d; gate ANI >= %g, fragments >= %d"
          % (n, L, a.cluster_size or n, sk.profile_bins(), p.fragLen - 20, len(sk.chunks()), a.replicates, a.boot_seed, a.min_ani, a.min_fragments), flush=True)
    wall, dev, red = ({s: [] for s in ("off", "on")} for _ in range(3))
    got = {}
    for turn in range(a.reps + 1):                                   # (the first turn warms up)
        for state in ("off", "on"):
            if state == "on":
                sk.boot_begin(a.replicates, a.boot_seed, a.min_ani, a.min_fragments)
            e.reset_counters()
            w, d = timed_once(lambda: got.__setitem__(state, sk.map_cgi_batch(genomes, 0)))
            ms = e.counters()["msReduce"]
            if state == "on":
                got["boot"] = sk.boot_take()
                sk.boot_end()
            if turn:
                wall[state].append(w)
                dev[state].append(d)
                red[state].append(ms / 1e3)
    assert np.array_equal(got["off"], got["on"]), "the rows differ with the mode on"
    (rec, sums), rows = got["boot"], got["on"]
    gated = (rows["countSeq"] >= a.min_fragments) & (rows["identity"] >= np.float32(a.min_ani))
    assert len(rec) == int(gated.sum()) and np.array_equal(rec["count"], rows["countSeq"][gated].astype(np.uint32))
    assert sums.shape == (len(rec), a.replicates) and (rec["replicates"] == a.replicates).all()
    med = lambda v: float(np.median(v))
    for state in ("off", "on"):
        print("boot %-3s: call by HIP events %.3f .. %.3f ms median %.3f ms   wall median %.3f ms   msReduce %.3f .. %.3f ms median %.3f ms   %d rows"
              % (state, min(dev[state]) * 1e3, max(dev[state]) * 1e3, med(dev[state]) * 1e3, med(wall[state]) * 1e3, min(red[state]) * 1e3, max(red[state]) * 1e3,
                 med(red[state]) * 1e3, len(got[state])), flush=True)
    extra = med(red["on"]) - med(red["off"])
    print("on / off by the medians of the HIP events: %.4f (spread %.4f .. %.4f)   the new work (msReduce on - off): %.3f ms = %.2f %% of the call with the mode on; "
          "msReduce with the mode off (memset, k_oneway_bins, k_pair_reduce): %.3f ms"
          % (med(dev["on"]) / med(dev["off"]), min(dev["on"]) / max(dev["off"]), max(dev["on"]) / min(dev["off"]), extra * 1e3, 100.0 * extra / med(dev["on"]),
             med(red["off"]) * 1e3), flush=True)
    drawn = sums.min(axis=1) != sums.max(axis=1) if len(rec) else np.zeros(0, bool)       # (a pair with one distinct value skips the draws)
    cells = int(rec["count"].sum(dtype=np.uint64))
    print("records: %d (%.1f MB of records and sums to the host), %d cells; at least %d pairs with %d cells drew: >= %.3e draws per call"
          % (len(rec), len(rec) * (24 + 8 * a.replicates) / 1e6, cells, int(drawn.sum()), int(rec["count"][drawn].sum(dtype=np.uint64)),
             float(a.replicates) * float(rec["count"][drawn].sum(dtype=np.uint64))), flush=True)
    if len(rec):
        from fastani_amd.api import boot_identity
        ident = boot_identity(rec, sums)
        width = ident.max(axis=1) - ident.min(axis=1)
        print("records: count %d .. %d; range of the replicate identities of a pair %.4f .. %.4f (median %.4f)"
              % (int(rec["count"].min()), int(rec["count"].max()), float(width.min()), float(width.max()), float(np.median(width))), flush=True)
    sk.close()


if __name__ == "__main__":
    main()
