"""Cases for the per-bin conservation profile (kernels/profile.hpp: k_profile_bins, k_profile_queries; ani_sketch_profile_begin / _bins /
_read / _end in engine_map.hip), shared by the GPU tests (-m gpu, product library) and the CPU-emulation tests (not gpu, tests/emu
build): test_profile.py.

The reference is a numpy restatement of rules 1 - 4 of include/ani_abi.h, written here from a mapping list: the 1-way winner per
(fragment, reference genome), its bin, the per-bin maximum per query (the cell), then the gate and the integer sums.  The oracle gives
rows, not bins, so the restatement is first held to the oracle: the rows derived from its cells (the count of a genome's cells and
their float32 mean in (contig, bin) order) must be the oracle's rows bit for bit.  Every comparison is on bits; there is no tolerance.

The synthetic lists, the reference layout (genomes of 1, 63, 64, 65, 128, 129 and 3 bins: 453 bins, two 256-bin workgroups of
k_profile_bins, the second partial, genome borders inside a workgroup) and the engines are those of reduce_cases.py."""
import numpy as np

import reduce_cases as rc
from fastani_amd.api import BINPROFILE_DT, CGI_DT, AniError, Sketch
from parity_cases import mutate, rng_genome

ERR_ARG = rc.ERR_ARG
LISTS_ONE = ("random", "ties", "bin_edges", "dense", "last_bin_only", "hot_bin", "n1", "n0")
LISTS_MANY = ("random", "ties", "bin_edges", "dense", "hot_bin")
LISTS_RESTATE = ("random", "ties", "bin_edges", "dense", "hot_bin")
LISTS_GATE = ("random", "ties", "bin_edges", "dense")
FIX = 1048576.0                                          # 2^20


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


class Bins:
    """rule 1 over the contig tables of a reference set"""

    def __init__(self, contig_len, contig_genome, frag_len):
        self.bin_w = frag_len - 20
        self.contig_len = np.asarray(contig_len, dtype=np.int64)
        self.contig_genome = np.asarray(contig_genome, dtype=np.int64)
        self.contig_start = np.concatenate([[0], np.cumsum(self.contig_len // self.bin_w + 1)]).astype(np.int64)
        self.n_bins = int(self.contig_start[-1])
        self.n_genomes = int(self.contig_genome.max()) + 1
        first = np.searchsorted(self.contig_genome, np.arange(self.n_genomes + 1))      # contigs of a genome are consecutive
        self.genome_start = self.contig_start[first]


def bins_of(lay):
    return Bins(lay.contig_len, lay.contig_genome, lay.frag_len)


def cells(b, maps):
    """rule 2 for ONE query: uint32[nBins], the identity bits of every cell, 0 = empty"""
    out = np.zeros(b.n_bins, dtype=np.uint32)
    if len(maps) == 0:
        return out
    frag = maps["querySeqId"].astype(np.int64)
    seq = maps["refSeqId"].astype(np.int64)
    pos = maps["refStartPos"].astype(np.int64)
    idb = bits(maps["nucIdentity"]).astype(np.int64)
    gen = b.contig_genome[seq]
    o = np.lexsort((pos, seq, idb, gen, frag))           # the winner of a (fragment, genome) group is its last element
    last = np.ones(len(o), dtype=bool)
    last[:-1] = (frag[o][1:] != frag[o][:-1]) | (gen[o][1:] != gen[o][:-1])
    w = o[last]
    np.maximum.at(out, b.contig_start[seq[w]] + pos[w] // b.bin_w, idb[w].astype(np.uint32))
    return out


def rows_of(b, cell, total, qid):
    """the rows of one query from its cells: per genome with a cell, their count and their float32 mean, added in bin order"""
    rows = []
    for g in range(b.n_genomes):
        c = cell[b.genome_start[g]:b.genome_start[g + 1]]
        c = c[c != 0].view(np.float32)
        if len(c) == 0:
            continue
        s = np.float32(0.0)
        for x in c:
            s = np.float32(s + x)
        rows.append((g, qid, len(c), total, np.float32(s / np.float32(len(c)))))
    return np.array(rows, dtype=CGI_DT)


def gate_bits(min_identity):
    return 0 if float(min_identity) == 0.0 else int(bits(min_identity))


class Profile:
    """rules 3 and 4: the accumulators, and what ani_sketch_profile_read gives for them"""

    def __init__(self, b, min_identity=0.0, min_fragments=1):
        self.b, self.min_bits, self.min_fragments = b, gate_bits(min_identity), int(min_fragments)
        self.count = np.zeros(b.n_bins, dtype=np.uint64)
        self.sum = np.zeros(b.n_bins, dtype=np.uint64)
        self.min = np.full(b.n_bins, 0xffffffff, dtype=np.uint32)
        self.max = np.zeros(b.n_bins, dtype=np.uint32)
        self.queries = np.zeros(b.n_genomes, dtype=np.uint32)
        self.gated_count_seq = np.zeros(b.n_genomes, dtype=np.int64)       # the countSeq of the rows that passed, per genome

    def passes(self, row):
        return int(row["countSeq"]) >= self.min_fragments and int(bits(row["identity"])) >= self.min_bits

    def add(self, maps):
        """one query genome"""
        b = self.b
        cell = cells(b, maps)
        for row in rows_of(b, cell, 0, 0):
            if not self.passes(row):
                continue
            g = int(row["refGenomeId"])
            self.queries[g] += 1
            self.gated_count_seq[g] += int(row["countSeq"])
            sl = slice(int(b.genome_start[g]), int(b.genome_start[g + 1]))
            c = cell[sl]
            on = c != 0
            self.count[sl] += on.astype(np.uint64)
            fix = np.rint(c.view(np.float32).astype(np.float64) * FIX).astype(np.uint64)       # round half even
            self.sum[sl] += np.where(on, fix, 0).astype(np.uint64)
            self.min[sl] = np.where(on, np.minimum(self.min[sl], c), self.min[sl])
            self.max[sl] = np.maximum(self.max[sl], c)
        return self

    def add_many(self, maps, frag_start):
        for q in range(len(frag_start) - 1):
            self.add(maps[(maps["querySeqId"] >= frag_start[q]) & (maps["querySeqId"] < frag_start[q + 1])])
        return self

    def bins(self):
        out = np.zeros(self.b.n_bins, dtype=BINPROFILE_DT)
        out["count"] = self.count
        out["sum"] = self.sum
        out["minIdentity"] = np.where(self.count > 0, self.min, 0).astype(np.uint32).view(np.float32)
        out["maxIdentity"] = self.max.view(np.float32)
        return out


def same_profile(got, exp):
    """(bins, queries) against a Profile, the whole records as bits"""
    gb, gq = got
    eb = exp.bins()
    assert gb.dtype == BINPROFILE_DT and gb.shape == eb.shape, (gb.shape, eb.shape)
    if not np.array_equal(gb.view("<u4"), eb.view("<u4")):
        bad = np.flatnonzero((gb.view("<u4").reshape(-1, 6) != eb.view("<u4").reshape(-1, 6)).any(axis=1))
        raise AssertionError("%d bins differ, the first at %d: got %r, expected %r" % (len(bad), bad[0], gb[bad[0]], eb[bad[0]]))
    assert np.array_equal(gq, exp.queries), (gq, exp.queries)
    # the invariant: per genome, the counts of its bins add up to the countSeq of its rows that passed the gate
    b = exp.b
    per_genome = np.add.reduceat(gb["count"].astype(np.int64), b.genome_start[:-1])
    assert np.array_equal(per_genome, exp.gated_count_seq), (per_genome, exp.gated_count_seq)
    return True


def read_raw(sk):
    bins, queries = sk.profile_read()
    return bins.tobytes() + queries.tobytes()


def expect_error(fn, what, code=ERR_ARG):
    try:
        out = fn()
    except AniError as e:
        assert e.code == code, (what, e)
    else:
        raise AssertionError("%s: accepted, %r" % (what, out))


# ---- the restatement against the oracle (CPU only, no engine) ----
_osk = {}


def oracle_sketch(frag_len):
    """the oracle's sketch of the layout's sequences; its rows depend on the contig tables only, so any window does"""
    if frag_len not in _osk:
        lay = rc.Layout(frag_len)
        _osk[frag_len] = rc.orc.Sketch(lay.sequences(), rc.K, 24)
    return _osk[frag_len]


def case_restatement(frag_len, name):
    lay = rc.Layout(frag_len)
    b = bins_of(lay)
    maps, frags = rc.LISTS[name][0](lay)
    exp = oracle_sketch(frag_len).compute_cgi(maps, frags, 3, frag_len)
    got = rows_of(b, cells(b, maps), frags, 3)
    assert len(exp) >= 1 and rc.same_rows(got, exp), "%s, fragLen %d:\n%r\n%r" % (name, frag_len, got, exp)
    # and over several queries of one list, as the many-queries cases cut it
    start = rc.split_queries(frags, 5, 5)
    for q in range(5):
        mine = maps[(maps["querySeqId"] >= start[q]) & (maps["querySeqId"] < start[q + 1])]
        exp = oracle_sketch(frag_len).compute_cgi(mine, start[q + 1] - start[q], q, frag_len)
        assert rc.same_rows(rows_of(b, cells(b, mine), start[q + 1] - start[q], q), exp), (name, frag_len, q)


# ---- layout ----
def case_layout(ref):
    lay = ref.lay
    b = bins_of(lay)
    assert ref.sk.profile_bins() == int(lay.contig_bins.sum()) == b.n_bins == 453
    contig_start, genome_start = ref.sk.profile_layout()
    assert contig_start.dtype == np.int64 and genome_start.dtype == np.int64
    assert np.array_equal(contig_start, np.concatenate([[0], np.cumsum(lay.contig_bins)]))
    assert tuple(int(x) for x in np.diff(genome_start)) == rc.BIN_TOTALS and np.array_equal(genome_start, b.genome_start)
    assert b.n_bins > 256 and b.n_bins % 256 != 0 and any(0 < int(x) % 256 for x in genome_start[1:-1])


# ---- one query: ani_compute_cgi ----
def case_one_query(ref, name):
    lay, sk = ref.lay, ref.sk
    b = bins_of(lay)
    maps, frags = rc.LISTS[name][0](lay)
    exp_rows = ref.expected(maps, frags, 4)
    exp = Profile(b).add(maps)
    cell = cells(b, maps)
    for order in (rc.in_order, rc.shuffled):
        sk.profile_begin(0.0, 1)
        got_rows = sk.compute_cgi(order(maps), frags, 4)
        got = sk.profile_read()
        sk.profile_end()
        assert rc.same_rows(got_rows, exp_rows), (name, order.__name__)
        assert same_profile(got, exp), (name, order.__name__)
        gb = got[0]
        assert set(np.unique(gb["count"])) <= {0, 1}
        assert np.array_equal(gb["minIdentity"].view(np.uint32), cell) and np.array_equal(gb["maxIdentity"].view(np.uint32), cell)
        assert np.array_equal(got[1], np.isin(np.arange(b.n_genomes), exp_rows["refGenomeId"]).astype(np.uint32))


# ---- several queries in one table: ani_reduce_check ----
def oracle_gate(ref, maps, start):
    """(minIdentity, minFragments): the medians of the oracle rows' identity bits and countSeq (the upper median: a row's own value, so
    that one row sits on the threshold bit for bit); asserts from the oracle rows that either condition has both sides"""
    rows = rc.expected_many(ref, maps, start, 0)
    idb, cnt = np.sort(bits(rows["identity"])), np.sort(rows["countSeq"])
    thr_id, thr_cnt = idb[len(idb) // 2], int(cnt[len(cnt) // 2])
    rb = bits(rows["identity"])
    assert (rb >= thr_id).any() and (rb < thr_id).any() and (rb == thr_id).any(), "the identity gate does not divide the rows"
    assert (rows["countSeq"] >= thr_cnt).any() and (rows["countSeq"] < thr_cnt).any(), "the fragment gate does not divide the rows"
    both = (rb >= thr_id) & (rows["countSeq"] >= thr_cnt)
    assert both.any() and not both.all()
    return thr_id.view(np.float32), thr_cnt


def case_many(ref, name, gated=False):
    """the loops of reduce_cases.case_many with a profile around every call"""
    lay, sk = ref.lay, ref.sk
    b = bins_of(lay)
    maps0, frags = rc.LISTS[name][0](lay)
    # (the gated runs take 3 and 5 queries: one or two queries give too few rows for the medians to leave a pair on either side)
    for n_query in ((3, 5) if gated else (1, 2, 5)):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (None, 9), (0, 0), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (3, 1000), (5, 0)):
                    continue
                maps, start = rc.with_empty(maps0, rc.split_queries(frags, n_query, n_query), first, last)
                gate = oracle_gate(ref, maps, start) if gated else (0.0, 1)
                exp_rows = rc.expected_many(ref, maps, start, 7)
                exp = Profile(b, *gate).add_many(maps, start)
                passing = sum(exp.passes(r) for r in exp_rows)
                assert int(exp.queries.sum()) == passing and (not gated or 0 < passing < len(exp_rows))
                for order in (rc.in_order, rc.shuffled):
                    sk.profile_begin(*gate)
                    got_rows = rc.reduce_check(ref, order(maps), start, genome_base, 7)
                    got = sk.profile_read()
                    sk.profile_end()
                    what = "%s, fragLen %d, %d queries %r, genomeBase %d, gate %r, %s" % (name, lay.frag_len, n_query, start, genome_base, gate, order.__name__)
                    assert rc.same_rows(got_rows, exp_rows), what
                    assert same_profile(got, exp), what
                    if name == "hot_bin" and not gated:
                        assert int(got[0]["count"].max()) == n_query and int((got[0]["count"] > 0).sum()) == 1, what


def case_gate_edges(ref):
    """the gate's own edges on `random` over 5 queries: -0.0 is 0; a row on the identity threshold contributes and the next float above
    it shuts it out; minIdentity 100 and a minFragments above every countSeq leave an empty profile"""
    lay, sk = ref.lay, ref.sk
    b = bins_of(lay)
    maps, frags = rc.list_random(lay)
    start = rc.split_queries(frags, 5, 5)
    rows = rc.expected_many(ref, maps, start, 0)
    thr = np.sort(rows["identity"])[len(rows) // 2]
    above = np.nextafter(thr, np.float32(200.0))
    n_at = int((bits(rows["identity"]) >= bits(thr)).sum())
    n_above = int((bits(rows["identity"]) >= bits(above)).sum())
    assert n_at > n_above > 0
    for gate, n in (((-0.0, 1), len(rows)), ((thr, 1), n_at), ((above, 1), n_above), ((100.0, 1), 0), ((0.0, int(rows["countSeq"].max()) + 1), 0),
                    ((0.0, int(rows["countSeq"].max())), None)):
        sk.profile_begin(*gate)
        rc.reduce_check(ref, maps, start, 0, 0)
        got = sk.profile_read()
        sk.profile_end()
        exp = Profile(b, *gate).add_many(maps, start)
        assert same_profile(got, exp), gate
        assert n is None or int(got[1].sum()) == n, (gate, got[1], n)
        if n == 0:
            assert not got[0].view("<u4").any()           # an empty bin reads {0, 0.0f, 0.0f, 0, 0}


# ---- life cycle and arguments ----
def case_life_cycle(ref):
    lay, sk = ref.lay, ref.sk
    b = bins_of(lay)
    a_maps, a_frags = rc.list_random(lay)
    b_maps, b_frags = rc.list_ties(lay)
    a_maps = rc.in_order(a_maps)
    a_rows, b_rows = ref.expected(a_maps, a_frags, 1), ref.expected(b_maps, b_frags, 2)
    start = rc.split_queries(b_frags, 5, 5)
    many_rows = rc.expected_many(ref, b_maps, start, 0)

    # two calls in either order; read twice
    sk.profile_begin()
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), a_rows) and rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 0), many_rows)
    first = sk.profile_read()
    assert read_raw(sk) == read_raw(sk) == first[0].tobytes() + first[1].tobytes()
    sk.profile_begin()
    assert rc.same_rows(rc.reduce_check(ref, b_maps, start, 0, 0), many_rows) and rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), a_rows)
    second = sk.profile_read()
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert same_profile(first, Profile(b).add(a_maps).add_many(b_maps, start))
    # a genome mapped twice counts twice; ani_map_query-free calls only: nothing else adds
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), a_rows)
    assert same_profile(sk.profile_read(), Profile(b).add(a_maps).add_many(b_maps, start).add(a_maps))

    # begin again: zeroes, and takes the new gate
    gate = oracle_gate(ref, b_maps, start)
    sk.profile_begin(*gate)
    zero = sk.profile_read()
    assert not zero[0].view("<u4").any() and not zero[1].any()
    rc.reduce_check(ref, b_maps, start, 0, 0)
    assert same_profile(sk.profile_read(), Profile(b, *gate).add_many(b_maps, start))

    # every refused list leaves the profile as it was
    sk.profile_begin()
    sk.compute_cgi(a_maps, a_frags, 1)
    before = read_raw(sk)
    for i, (what, field, value) in enumerate(rc.bad_mappings(lay)):
        at = (0, len(a_maps) // 2, len(a_maps) - 1)[i % 3]
        bad = a_maps.copy()
        bad[field][at] = lay.contig_len[bad["refSeqId"][at]] + 1 if isinstance(value, str) else value
        expect_error(lambda: sk.compute_cgi(bad, a_frags, 1), what)
        assert read_raw(sk) == before, "after " + what
    outside = b_maps.copy()
    outside["querySeqId"][len(b_maps) // 2] = b_frags
    expect_error(lambda: rc.reduce_check(ref, outside, start, 0, 0), "querySeqId outside the table")
    assert read_raw(sk) == before

    # end: read and end are refused, mapping works and returns the same rows
    sk.profile_end()
    expect_error(sk.profile_read, "read after end")
    expect_error(sk.profile_end, "end after end")
    assert rc.same_rows(sk.compute_cgi(a_maps, a_frags, 1), a_rows) and rc.same_rows(sk.compute_cgi(b_maps, b_frags, 2), b_rows)
    assert sk.profile_bins() == b.n_bins                  # with or without a begin


def case_arguments(ref):
    sk, lib = ref.sk, ref.engine.lib
    chk = ref.engine._chk
    maps, frags = rc.list_random(ref.lay)
    f32 = np.float32
    expect_error(sk.profile_read, "read without begin")
    expect_error(sk.profile_end, "end without begin")
    for what, v in (("negative", -1.0), ("just below 0", -float(np.finfo(f32).tiny)), ("above 100", float(np.nextafter(f32(100.0), f32(200.0)))),
                    ("NaN", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        expect_error(lambda: sk.profile_begin(v, 1), "minIdentity " + what)
    for n in (0, -1, -2 ** 31):
        expect_error(lambda: sk.profile_begin(50.0, n), "minFragments %d" % n)
    expect_error(sk.profile_read, "read after a refused begin")
    # a refused begin leaves a running profile and its gate alone
    sk.profile_begin(0.0, 1)
    sk.compute_cgi(maps, frags, 0)
    before = read_raw(sk)
    expect_error(lambda: sk.profile_begin(101.0, 1), "minIdentity 101")
    expect_error(lambda: sk.profile_begin(0.0, 0), "minFragments 0")
    assert read_raw(sk) == before
    # null pointers
    import ctypes
    n = ctypes.c_uint64()
    expect_error(lambda: chk(lib.ani_sketch_profile_begin(None, 0.0, 1)), "begin(null)")
    expect_error(lambda: chk(lib.ani_sketch_profile_bins(None, ctypes.byref(n))), "bins(null)")
    expect_error(lambda: chk(lib.ani_sketch_profile_bins(sk.h, None)), "bins(sk, null)")
    expect_error(lambda: chk(lib.ani_sketch_profile_read(None, None, None)), "read(null)")
    expect_error(lambda: chk(lib.ani_sketch_profile_end(None)), "end(null)")
    # either output of read may be null
    chk(lib.ani_sketch_profile_read(sk.h, None, None))
    q = np.zeros(len(rc.BIN_TOTALS), dtype=np.uint32)
    chk(lib.ani_sketch_profile_read(sk.h, None, q.ctypes.data))
    bins = np.zeros(sk.profile_bins(), dtype=BINPROFILE_DT)
    chk(lib.ani_sketch_profile_read(sk.h, bins.ctypes.data, None))
    assert bins.tobytes() + q.tobytes() == before
    # the limits of the range are accepted
    sk.profile_begin(100.0, 2 ** 31 - 1)
    sk.profile_begin(0.0, 1)
    sk.profile_end()


# ---- end to end: the mapper's own cells ----
E2E_K, E2E_FRAG_LEN, E2E_LEN = 16, 1000, 60000
E2E_GATE = (95.0, 10)


def e2e_genomes(n=E2E_LEN):
    """4 reference and 6 query genomes of about n bases in two families; queries at several distances, one with a foreign island, one short"""
    fa, fb = rng_genome(7101, n), rng_genome(7102, n + n // 40)
    refs = [[fa], [mutate(fa, 0.02, 1)[:2 * n // 3], mutate(fa, 0.02, 2)[2 * n // 3:]], [fb], [mutate(fb, 0.03, 3)]]
    island = mutate(fa, 0.01, 4)
    island[n // 3:n // 3 + n // 5] = rng_genome(7103, n // 5)
    queries = [[mutate(fa, 0.01, 5)], [island], [mutate(fa, 0.08, 6)], [mutate(fb, 0.015, 7)], [mutate(fb, 0.03, 8)[:n // 7]], [mutate(fb, 0.1, 9)]]
    return refs, queries


class EndToEnd:
    """the inputs, and the restatement over each query's ani_map_query mappings, made once per half by the default engine"""

    def __init__(self, engine):
        self.refs, self.queries = e2e_genomes()
        self.p = engine.params(E2E_K, E2E_FRAG_LEN)
        sk = Sketch(engine, self.p, self.refs)
        self.n_minimizers = sk.stats()["minimizers"]
        contig_len = [len(c) for g in self.refs for c in g]
        contig_genome = [g for g, cs in enumerate(self.refs) for _ in cs]
        self.b = Bins(contig_len, contig_genome, E2E_FRAG_LEN)
        assert 200 < self.b.n_bins < 1000 and sk.profile_bins() == self.b.n_bins
        self.exp = Profile(self.b, *E2E_GATE)
        open_gate = Profile(self.b)
        rows = []
        for qi, q in enumerate(self.queries):
            maps, total = sk.map_query(q)
            self.exp.add(maps)
            open_gate.add(maps)
            rows.append(sk.compute_cgi(maps, total, qi))
        self.rows = np.concatenate(rows)
        sk.close()
        # the gate divides the pairs, and both conditions bite
        assert 0 < int(self.exp.queries.sum()) < int(open_gate.queries.sum()) == len(self.rows)
        assert (self.rows["countSeq"] < E2E_GATE[1]).any() and (self.rows["identity"] < E2E_GATE[0]).any()
        assert int((self.exp.count > 1).sum()) > 50 and int((self.exp.count == 1).sum()) > 50 and int((self.exp.count == 0).sum()) > 0

    def run(self, engine, config):
        sk = Sketch(engine, self.p, self.refs)
        if config in ("chunked", "streamed"):
            assert len(sk.chunks()) >= 3 and sk.residency()["streaming"] == (config == "streamed"), (sk.chunks(), sk.residency())
        else:
            assert len(sk.chunks()) == 1
        sk.profile_begin(*E2E_GATE)
        rows = sk.map_cgi_batch(self.queries, 0)
        assert rc.same_rows(rows, self.rows), config
        assert same_profile(sk.profile_read(), self.exp), config + ", map_cgi_batch"
        # kept fragment sets, in two sets of three genomes
        sk.profile_begin(*E2E_GATE)
        sets = [engine.fragment_set(self.p, self.queries[:3]), engine.fragment_set(self.p, self.queries[3:])]
        rows = sk.map_cgi_fragsets(sets, [0, 3])
        assert rc.same_rows(rows, self.rows), config
        assert same_profile(sk.profile_read(), self.exp), config + ", map_cgi_fragsets"
        for s in sets:
            s.close()
        sk.close()                                       # a sketch destroyed with a profile on releases it


# ---- the command line: --profile ----
def profile_lines(names, genomes, frag_len, bins, queries):
    """the .profile file of the references `genomes` (lists of contigs) named `names`, from the Python API's profile of one sketch that
    holds them in this order"""
    bin_w, out, b = frag_len - 20, [], 0
    for r, contigs in enumerate(genomes):
        for c, contig in enumerate(contigs):
            n = len(contig)
            for j in range(n // bin_w + 1):
                x = bins[b]
                b += 1
                start, covered = j * bin_w, int(x["count"])
                if start > n - frag_len and not covered:
                    continue                              # a contig's tail that cannot hold the start of a whole fragment
                head = "%s\t%d\t%d\t%d\t%d\t%d" % (names[r], c + 1, start, min((j + 1) * bin_w, n), int(queries[r]), covered)
                if covered:
                    mean = np.float32(float(x["sum"]) / FIX / covered)
                    out.append(head + "\t%g\t%g\t%g" % (float(mean), float(x["minIdentity"]), float(x["maxIdentity"])))
                else:
                    out.append(head + "\tNA\tNA\tNA")
    assert b == len(bins)
    return out


CLI_LEN = 24000                                          # 24 fragments a genome: the short query has 3, under the gate's 10


CLI_MODES = {
    # name -> (all-vs-all, extra options): the streaming path with one list and with two, and the split path (-s) on two reference splits
    "all_vs_all": (True, []),
    "lists": (False, []),
    "split": (False, ["-t", "2", "-s"]),
}


def case_cli(binary, engine, tmp, mode):
    import os
    import subprocess
    all_vs_all, extra = CLI_MODES[mode]
    refs, queries = e2e_genomes(CLI_LEN)
    if all_vs_all:
        refs = queries = refs + queries[:2]
    files = {}

    def write(kind, genomes):
        paths = []
        for i, g in enumerate(genomes):
            key = id(g)
            if key not in files:
                files[key] = os.path.join(tmp, "%s%d.fa" % (kind, i))
                rc.orc.write_fasta(files[key], g, names=["%s%d_%d" % (kind, i, j) for j in range(len(g))])
            paths.append(files[key])
        lst = os.path.join(tmp, kind + ".txt")
        open(lst, "w").write("\n".join(paths) + "\n")
        return paths, lst

    ref_paths, rl = write("r", refs)
    _, ql = write("q", queries)
    base = [binary, "--ql", ql, "--rl", rl, "--fragLen", str(E2E_FRAG_LEN), "-k", str(E2E_K), "--matrix"] + extra
    gate = ["--profileMinANI", str(E2E_GATE[0]), "--profileMinFragments", str(E2E_GATE[1])]
    plain, prof = os.path.join(tmp, "plain.out"), os.path.join(tmp, "prof.out")
    for out, opts in ((plain, []), (prof, ["--profile"] + gate)):
        r = subprocess.run(base + ["-o", out] + opts, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    # every other file is what it was
    produced = sorted(f[len("plain.out"):] for f in os.listdir(tmp) if f.startswith("plain.out"))
    assert produced == ["", ".matrix"] and sorted(f[len("prof.out"):] for f in os.listdir(tmp) if f.startswith("prof.out")) == ["", ".matrix", ".profile"]
    for suffix in produced:
        assert open(plain + suffix, "rb").read() == open(prof + suffix, "rb").read(), suffix
    assert len(open(plain).read().splitlines()) >= 6
    # the file against the Python API's profile at the same gate
    p = engine.params(E2E_K, E2E_FRAG_LEN)
    sk = Sketch(engine, p, refs)
    sk.profile_begin(*E2E_GATE)
    sk.map_cgi_batch(queries, 0)
    bins, qn = sk.profile_read()
    sk.close()
    exp = profile_lines(ref_paths, refs, E2E_FRAG_LEN, bins, qn)
    got = open(prof + ".profile").read().splitlines()
    assert got == exp, "%s: %d lines, expected %d; first difference %r" % (mode, len(got), len(exp), next(((a, b) for a, b in zip(got, exp) if a != b), None))
    covered = [int(line.split("\t")[5]) for line in got]
    assert any(c > 1 for c in covered) and any(c == 0 for c in covered) and any(line.endswith("\tNA\tNA\tNA") for line in got)
    # the default gate, 95 and 50, when neither option is given
    if mode == "lists":
        r = subprocess.run(base + ["-o", prof, "--profile"], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        sk = Sketch(engine, p, refs)
        sk.profile_begin(95.0, 50)
        sk.map_cgi_batch(queries, 0)
        bins, qn = sk.profile_read()
        sk.close()
        assert open(prof + ".profile").read().splitlines() == profile_lines(ref_paths, refs, E2E_FRAG_LEN, bins, qn)
        # the dependent options are refused by name without --profile, and their ranges hold
        for opts, msg in ((["--profileMinANI", "90"], b"--profileMinANI needs --profile"), (["--profileMinFragments", "5"], b"--profileMinFragments needs --profile"),
                          (["--profile", "--profileMinANI", "0"], b"--profileMinANI takes"), (["--profile", "--profileMinANI", "100.5"], b"--profileMinANI takes"),
                          (["--profile", "--profileMinFragments", "0"], b"--profileMinFragments takes")):
            r = subprocess.run(base + ["-o", os.path.join(tmp, "refused.out")] + opts, capture_output=True)
            assert r.returncode == 1 and msg in r.stderr, (opts, r.stderr[-500:])
        assert not os.path.exists(os.path.join(tmp, "refused.out"))
