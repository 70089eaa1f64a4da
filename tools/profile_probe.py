"""Cost of the per-bin conservation profile on the GPU: ani_map_cgi_batch of synthetic genomes against
themselves with the profile off and on, same process, same sketch, same inputs, the two taken in turns (off, on, off, on, ...) so that
a drift of the machine meets both; 1 warm-up turn + --reps timed turns, medians reported.

    python tools/profile_probe.py                              200 genomes of 1 Mbp in ONE cluster (a species-dense set: every pair has a row)
    python tools/profile_probe.py --genomes 1000 --genome-len 5000000 --cluster-size 20      the benchmark's set
    python tools/profile_probe.py --min-ani 95 --min-fragments 50                           the gate (the command line's defaults)

Per state: the call by the wall clock and by HIP events around it (it returns after its last copy), and the reducer's own HIP-event
timer (ani_counters_t.msReduce: the bin table's memset, k_oneway_bins, k_pair_reduce and, with a profile, k_profile_bins and
k_profile_queries).  The kernels' share is the difference of the msReduce medians over the median of the call with the profile on.
Also: the bytes of bin table k_profile_bins read (4 x queries x bins, per sub-batch and index chunk), and a core-genome size from the
profile: the bins with count >= 0.95 x queries of their genome.
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
    ap.add_argument("--min-ani", type=float, default=95.0)
    ap.add_argument("--min-fragments", type=int, default=50)
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
    n_bins = sk.profile_bins()
    _, genome_start = sk.profile_layout()
    print("profile_probe: %d genomes of %d bases, clusters of %d; %d bins of %d bases, %d index chunk(s); gate ANI >= %g, fragments >= %d"
          % (n, L, a.cluster_size or n, n_bins, p.fragLen - 20, len(sk.chunks()), a.min_ani, a.min_fragments), flush=True)
    wall, dev, red, rows = ({s: [] for s in ("off", "on")} for _ in range(4))
    got = {}
    for turn in range(a.reps + 1):                                   # (the first turn warms up)
        for state in ("off", "on"):
            if state == "on":
                sk.profile_begin(a.min_ani, a.min_fragments)
            e.reset_counters()
            w, d = timed_once(lambda: got.__setitem__(state, sk.map_cgi_batch(genomes, 0)))
            ms = e.counters()["msReduce"]
            if state == "on":
                got["profile"] = sk.profile_read()
                sk.profile_end()
            if turn:
                wall[state].append(w)
                dev[state].append(d)
                red[state].append(ms / 1e3)
    assert np.array_equal(got["off"], got["on"]), "the rows differ with a profile"
    med = lambda v: float(np.median(v))
    for state in ("off", "on"):
        print("profile %-3s: call by HIP events %.3f .. %.3f ms median %.3f ms   wall median %.3f ms   msReduce %.3f .. %.3f ms median %.3f ms   %d rows"
              % (state, min(dev[state]) * 1e3, max(dev[state]) * 1e3, med(dev[state]) * 1e3, med(wall[state]) * 1e3, min(red[state]) * 1e3, max(red[state]) * 1e3,
                 med(red[state]) * 1e3, len(got[state])), flush=True)
    extra = med(red["on"]) - med(red["off"])
    table = 4.0 * n * n_bins
    print("on / off by the medians of the HIP events: %.4f (spread %.4f .. %.4f)   profile kernels (msReduce on - off): %.3f ms = %.2f %% of the call with the profile on"
          % (med(dev["on"]) / med(dev["off"]), min(dev["on"]) / max(dev["off"]), max(dev["on"]) / min(dev["off"]), extra * 1e3, 100.0 * extra / med(dev["on"])), flush=True)
    print("bin table read by k_profile_bins: %.3f GB per call%s" % (table / 1e9, "   (%.0f GB/s over the kernels' time)" % (table / 1e9 / extra) if extra > 0 else ""), flush=True)
    bins, queries = got["profile"]
    per_bin_queries = np.repeat(queries, np.diff(genome_start))
    core = (per_bin_queries > 0) & (bins["count"] >= 0.95 * per_bin_queries)
    print("profile: queries per reference %d .. %d; %d of %d bins covered at all; core genome (count >= 0.95 x queries): %d bins = %.1f %% = about %d bases per genome"
          % (int(queries.min()), int(queries.max()), int((bins["count"] > 0).sum()), n_bins, int(core.sum()), 100.0 * core.sum() / max(n_bins, 1),
             int(core.sum()) * (p.fragLen - 20) // max(n, 1)), flush=True)
    sk.close()


if __name__ == "__main__":
    main()
