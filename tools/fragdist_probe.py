"""Cost of the per-pair fragment identity distributions on the GPU: ani_map_cgi_batch of synthetic genomes
against themselves with the mode off and on, same process, same sketch, same inputs, the two taken in turns (off, on, off, on, ...) so
that a drift of the machine meets both; 1 warm-up turn + --reps timed turns, medians reported.

    python tools/fragdist_probe.py                              200 genomes of 1 Mbp in ONE cluster (a species-dense set: every pair has a row)
    python tools/fragdist_probe.py --genomes 1000 --genome-len 5000000 --cluster-size 20      the benchmark's set
    python tools/fragdist_probe.py --min-ani 95 --min-fragments 50                           a gate

Per state: the call by the wall clock and by HIP events around it (it returns after its last copy), and the reducer's own HIP-event
timer (ani_counters_t.msReduce: the bin table's memset, k_oneway_bins, k_pair_reduce and, with the mode on, k_fragdist_flags, the scan,
k_fragdist_list, k_fragdist_records and the copies of the records to the host).  The new work's share is the difference of the msReduce
medians.  Also: the number of records, the bytes the kernels read (the pair table once, the cells of every gated pair once in the first
walk and three times more in the select where the pair has more than one distinct value), and the same for k_pair_reduce (every
pair's cells once).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_EDGES = [float(e) for e in range(70, 100)] + [99.5, 99.9]


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
    n_bins = sk.profile_bins()
    print("fragdist_probe: %d genomes of %d bases, clusters of %d; %d bins of %d bases, %d index chunk(s); %d class edges; gate ANI >= %g, fragments >= %d"
          % (n, L, a.cluster_size or n, n_bins, p.fragLen - 20, len(sk.chunks()), len(DEFAULT_EDGES), a.min_ani, a.min_fragments), flush=True)
    wall, dev, red = ({s: [] for s in ("off", "on")} for _ in range(3))
    got = {}
    for turn in range(a.reps + 1):                                   # (the first turn warms up)
        for state in ("off", "on"):
            if state == "on":
                sk.fragdist_begin(DEFAULT_EDGES, a.min_ani, a.min_fragments)
            e.reset_counters()
            w, d = timed_once(lambda: got.__setitem__(state, sk.map_cgi_batch(genomes, 0)))
            ms = e.counters()["msReduce"]
            if state == "on":
                got["dist"] = sk.fragdist_take()
                sk.fragdist_end()
            if turn:
                wall[state].append(w)
                dev[state].append(d)
                red[state].append(ms / 1e3)
    assert np.array_equal(got["off"], got["on"]), "the rows differ with the mode on"
    rec, hist = got["dist"]
    rows = got["on"]
    gated = (rows["countSeq"] >= a.min_fragments) & (rows["identity"] >= np.float32(a.min_ani))
    assert len(rec) == int(gated.sum()) and np.array_equal(rec["count"], rows["countSeq"][gated].astype(np.uint32))
    assert np.array_equal(hist.sum(axis=1, dtype=np.uint64), rec["count"].astype(np.uint64))
    med = lambda v: float(np.median(v))
    for state in ("off", "on"):
        print("fragdist %-3s: call by HIP events %.3f .. %.3f ms median %.3f ms   wall median %.3f ms   msReduce %.3f .. %.3f ms median %.3f ms   %d rows"
              % (state, min(dev[state]) * 1e3, max(dev[state]) * 1e3, med(dev[state]) * 1e3, med(wall[state]) * 1e3, min(red[state]) * 1e3, max(red[state]) * 1e3,
                 med(red[state]) * 1e3, len(got[state])), flush=True)
    extra = med(red["on"]) - med(red["off"])
    print("on / off by the medians of the HIP events: %.4f (spread %.4f .. %.4f)   the new work (msReduce on - off): %.3f ms = %.2f %% of the call with the mode on; "
          "msReduce with the mode off (memset, k_oneway_bins, k_pair_reduce): %.3f ms"
          % (med(dev["on"]) / med(dev["off"]), min(dev["on"]) / max(dev["off"]), max(dev["on"]) / min(dev["off"]), extra * 1e3, 100.0 * extra / med(dev["on"]),
             med(red["off"]) * 1e3), flush=True)
    bins_per_genome = n_bins / max(n, 1)
    spread_out = int((rec["minIdentity"] != rec["maxIdentity"]).sum())       # the others skip the select's three walks
    pair_table, first, select = 8.0 * n * n, 4.0 * len(rec) * bins_per_genome, 3 * 4.0 * spread_out * bins_per_genome
    print("records: %d (%.1f MB on the host with their histograms), %d of them with more than one distinct value; read by the new kernels: pair table %.3f GB + "
          "first walk %.3f GB + select %.3f GB of cells = %.3f GB per call; k_pair_reduce reads %.3f GB"
          % (len(rec), (len(rec) * (40 + 4 * hist.shape[1])) / 1e6, spread_out, pair_table / 1e9, first / 1e9, select / 1e9, (pair_table + first + select) / 1e9,
             4.0 * n * n_bins / 1e9), flush=True)
    if len(rec):
        spread = rec["q3"] - rec["q1"]
        print("records: count %d .. %d; median identity %.3f .. %.3f; interquartile range %.3f .. %.3f (median %.3f)"
              % (int(rec["count"].min()), int(rec["count"].max()), float(rec["median"].min()), float(rec["median"].max()), float(spread.min()), float(spread.max()),
                 float(np.median(spread))), flush=True)
    sk.close()


if __name__ == "__main__":
    main()
