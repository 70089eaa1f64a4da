"""Cost of the paint records on the GPU: ani_map_cgi_batch of synthetic genomes against themselves with the mode
off and on, same process, same sketch, same inputs, the two taken in turns (off, on, off, on, ...) so that a drift of the machine meets
both; 1 warm-up turn + --reps timed turns, medians reported.

    python tools/paint_probe.py                              200 genomes of 1 Mbp in ONE cluster (a species-dense set: every fragment
                                                             has a winner in every genome, 200 group heads meet on each fragment)
    python tools/paint_probe.py --genomes 1000 --genome-len 5000000 --cluster-size 20      the benchmark's set

Per state: the call by the wall clock and by HIP events around it (it returns after its last copy), and the reducer's own HIP-event
timer (ani_counters_t.msReduce: the bin table's memset, k_oneway_bins, k_pair_reduce and, with the mode on, the state's memsets,
k_paint_best, k_paint_second, k_paint_flags, the scan, k_paint_records and the copies of the records to the host).  The new work's share is
the difference of the msReduce medians.  Also: the number of records, the bytes that reach the host (40 per record), and a check of the
records against the rows (a fragment's best genome has a row for its query, the fragments are in order, a second exists exactly where
more than one genome is hit).
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
    ap.add_argument("--seed", type=int, default=20260925)
    ap.add_argument("--show", type=int, default=3, help="records to print")
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
    print("paint_probe: %d genomes of %d bases, clusters of %d; %d index chunk(s)" % (n, L, a.cluster_size or n, len(sk.chunks())), flush=True)
    wall, dev, red = ({s: [] for s in ("off", "on")} for _ in range(3))
    got = {}
    for turn in range(a.reps + 1):                                   # (the first turn warms up)
        for state in ("off", "on"):
            if state == "on":
                sk.paint_begin()
            e.reset_counters()
            w, d = timed_once(lambda: got.__setitem__(state, sk.map_cgi_batch(genomes, 0)))
            ms = e.counters()["msReduce"]
            if state == "on":
                got["paint"] = sk.paint_take()
                sk.paint_end()
            if turn:
                wall[state].append(w)
                dev[state].append(d)
                red[state].append(ms / 1e3)
    assert np.array_equal(got["off"], got["on"]), "the rows differ with the mode on"
    rec, rows = got["paint"], got["on"]
    key = rec["qryGenomeId"].astype(np.int64) << 32 | rec["querySeqId"].astype(np.int64)
    assert (np.diff(key) > 0).all(), "the records are not in (query, fragment) order"
    pairs = set((rows["qryGenomeId"].astype(np.int64) << 32 | rows["refGenomeId"].astype(np.int64)).tolist())
    # (a best genome's 1-way winner fills a cell of the pair, so the pair has a row)
    assert all(int(k) in pairs for k in np.unique(rec["qryGenomeId"].astype(np.int64) << 32 | rec["refGenomeId"].astype(np.int64)))
    assert (rec["genomes"] >= 1).all() and ((rec["secondGenomeId"] >= 0) == (rec["genomes"] > 1)).all()
    med = lambda v: float(np.median(v))
    for state in ("off", "on"):
        print("paint %-3s: call by HIP events %.3f .. %.3f ms median %.3f ms   wall median %.3f ms   msReduce %.3f .. %.3f ms median %.3f ms   %d rows"
              % (state, min(dev[state]) * 1e3, max(dev[state]) * 1e3, med(dev[state]) * 1e3, med(wall[state]) * 1e3, min(red[state]) * 1e3, max(red[state]) * 1e3,
                 med(red[state]) * 1e3, len(got[state])), flush=True)
    extra = med(red["on"]) - med(red["off"])
    print("on / off by the medians of the HIP events: %.4f (spread %.4f .. %.4f)   the new work (msReduce on - off): %.3f ms = %.2f %% of the call with the mode on; "
          "msReduce with the mode off (memset, k_oneway_bins, k_pair_reduce): %.3f ms"
          % (med(dev["on"]) / med(dev["off"]), min(dev["on"]) / max(dev["off"]), max(dev["on"]) / min(dev["off"]), extra * 1e3, 100.0 * extra / med(dev["on"]),
             med(red["off"]) * 1e3), flush=True)
    print("records: %d (fragments with a best reference), %.1f MB to the host and on the host until taken; mean genomes per fragment %.2f, largest %d; "
          "%d fragments hit one genome only" % (len(rec), len(rec) * 40 / 1e6, float(rec["genomes"].mean()) if len(rec) else 0.0,
                                                 int(rec["genomes"].max()) if len(rec) else 0, int((rec["genomes"] == 1).sum())), flush=True)
    for r in rec[:a.show]:
        print("  qry %d querySeqId %d ref %d refSeqId %d refStartPos %d identity %.4f second %d secondIdentity %.4f genomes %d" % tuple(r)[:9], flush=True)
    sk.close()


if __name__ == "__main__":
    main()
