"""Cost of the synteny records on the GPU: ani_map_cgi_batch of synthetic genomes against themselves with the
mode off and on, same process, same sketch, same inputs, the two taken in turns (off, on, off, on, ...) so that a drift of the machine
meets both; 1 warm-up turn + --reps timed turns, medians reported.

    python tools/synteny_probe.py                              200 genomes of 1 Mbp in ONE cluster (a species-dense set: every pair has a row)
    python tools/synteny_probe.py --genomes 1000 --genome-len 5000000 --cluster-size 20      the benchmark's set
    python tools/synteny_probe.py --min-ani 95 --min-fragments 50                           a gate

Per state: the call by the wall clock and by HIP events around it (it returns after its last copy), and the reducer's own HIP-event
timer (ani_counters_t.msReduce: the bin table's memset, k_oneway_bins, k_pair_reduce and, with the mode on, k_hits_flags, the scans, the
owner table's memset, k_hits_owner, k_hits_claim, k_syn_list, k_syn_pairs, k_syn_compact and the copies of the records to the host).
The new work's share is the difference of the msReduce medians.  Also: the numbers of pair and block records, the bytes that reach the
host (48 per pair, 32 per block) beside the 24 bytes per hit the same pairs would send as hit records, and a check of the records
against the rows (a gated row has one pair record, count = countSeq, and the two identities of the pair record hold).
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
    ap.add_argument("--min-ani", type=float, default=0.0)
    ap.add_argument("--min-fragments", type=int, default=1)
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
    print("synteny_probe: %d genomes of %d bases, clusters of %d; %d bins of %d bases, %d index chunk(s); gate ANI >= %g, fragments >= %d"
          % (n, L, a.cluster_size or n, sk.profile_bins(), p.fragLen - 20, len(sk.chunks()), a.min_ani, a.min_fragments), flush=True)
    wall, dev, red = ({s: [] for s in ("off", "on")} for _ in range(3))
    got = {}
    for turn in range(a.reps + 1):                                   # (the first turn warms up)
        for state in ("off", "on"):
            if state == "on":
                sk.synteny_begin(a.min_ani, a.min_fragments)
            e.reset_counters()
            w, d = timed_once(lambda: got.__setitem__(state, sk.map_cgi_batch(genomes, 0)))
            ms = e.counters()["msReduce"]
            if state == "on":
                got["syn"] = sk.synteny_take()
                sk.synteny_end()
            if turn:
                wall[state].append(w)
                dev[state].append(d)
                red[state].append(ms / 1e3)
    assert np.array_equal(got["off"], got["on"]), "the rows differ with the mode on"
    (pairs, blocks), rows = got["syn"], got["on"]
    gated = rows[(rows["countSeq"] >= a.min_fragments) & (rows["identity"] >= np.float32(a.min_ani))]
    assert len(pairs) == len(gated) and np.array_equal(pairs["refGenomeId"], gated["refGenomeId"]) and np.array_equal(pairs["qryGenomeId"], gated["qryGenomeId"])
    assert np.array_equal(pairs["count"], gated["countSeq"].astype(np.uint32)) and int(pairs["blocks"].sum()) == len(blocks)
    i64 = lambda f: pairs[f].astype(np.int64)
    assert np.array_equal(i64("forward") + i64("reverse") + i64("breaks") + i64("contigBorders"), i64("count") - 1)
    assert np.array_equal(i64("blocks"), i64("breaks") + i64("contigBorders") + 1) and int(blocks["hits"].sum()) == int(pairs["count"].sum())
    med = lambda v: float(np.median(v))
    for state in ("off", "on"):
        print("synteny %-3s: call by HIP events %.3f .. %.3f ms median %.3f ms   wall median %.3f ms   msReduce %.3f .. %.3f ms median %.3f ms   %d rows"
              % (state, min(dev[state]) * 1e3, max(dev[state]) * 1e3, med(dev[state]) * 1e3, med(wall[state]) * 1e3, min(red[state]) * 1e3, max(red[state]) * 1e3,
                 med(red[state]) * 1e3, len(got[state])), flush=True)
    extra = med(red["on"]) - med(red["off"])
    print("on / off by the medians of the HIP events: %.4f (spread %.4f .. %.4f)   the new work (msReduce on - off): %.3f ms = %.2f %% of the call with the mode on; "
          "msReduce with the mode off (memset, k_oneway_bins, k_pair_reduce): %.3f ms"
          % (med(dev["on"]) / med(dev["off"]), min(dev["on"]) / max(dev["off"]), max(dev["on"]) / min(dev["off"]), extra * 1e3, 100.0 * extra / med(dev["on"]),
             med(red["off"]) * 1e3), flush=True)
    hits = int(pairs["count"].sum())
    print("records: %d pairs and %d blocks over %d hits, %.2f MB to the host (the same pairs' hit records: %.1f MB); largest block %d hits, %d reverse blocks, "
          "%d breaks, %d pairs of one block" % (len(pairs), len(blocks), hits, (len(pairs) * 48 + len(blocks) * 32) / 1e6, hits * 24 / 1e6,
                                                 int(pairs["largestBlock"].max()) if len(pairs) else 0, int(pairs["reverseBlocks"].sum()), int(pairs["breaks"].sum()),
                                                 int((pairs["blocks"] == 1).sum())), flush=True)
    for r in pairs[:a.show]:
        print("  " + " ".join("%s %d" % (f, int(r[f])) for f in pairs.dtype.names), flush=True)
    sk.close()


if __name__ == "__main__":
    main()
