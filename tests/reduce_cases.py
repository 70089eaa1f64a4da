"""Cases for the ANI reducer (kernels/reduce.hpp: k_oneway_bins, k_pair_reduce; ani_compute_cgi, reduce_stage and collect_rows in
engine_map.hip) on SYNTHETIC mapping lists, shared by the GPU tests (-m gpu, product library) and the CPU-emulation tests (not gpu,
tests/emu build): test_reducer.py.

The end-to-end cases feed the reducer what the project's own mapper emits: identities from a small table, ties resolved by whatever
positions come out, hardly a start position on a bin edge, no reference genome of exactly 64 or 65 bins.  Here the reference layout
and the lists are made to sit on the kernel's edges: the three-level tie-break (identity bits, refSeqId, refStartPos), the bin choice
refStartPos / (fragLen - 20) up to refStartPos == contigLen, the 64-bin slab edge of k_pair_reduce, the float summation order, the
row offset fragGenome - genomeBase, the (pairs + 3) / 4 grid, the column offset of an index chunk.

The reference is the oracle's plain sort-and-dedup form of computeCGI (orc.Sketch.compute_cgi).  Every comparison is on the bits of
the whole record array: the reducer is specified bit-exactly, no tolerance anywhere.

The reducer reads the contig and genome tables of a sketch only, so the sequences are random; a Layout chooses the contig lengths."""
import ctypes

import numpy as np

import orc
from fastani_amd.api import CGI_DT, MAPPING_DT, AniError, Sketch
from parity_cases import rng_genome

K = 16
FRAG_LENS = (1000, 3000)
BIN_TOTALS = (1, 63, 64, 65, 128, 129, 3)              # bins per reference genome: the slab edges of the 64-wide loop of k_pair_reduce
ERR_ARG = -1                                            # include/ani_abi.h
TPB = 256                                               # k_oneway_bins: threads per workgroup
TINY = (5, 15, 16, 17, 100, 500, 1, 33, 250, 700, 64)   # contigs of one bin; 1, 5 and 15 are shorter than a k-mer
# per genome: (k, d) -> a contig of k * binW + d bases, and the number of one-bin contigs behind them
SPEC = (
    ((), 1),
    (((10, -1), (10, 0), (10, 1), (9, -1), (9, 0), (9, 1)), 2),
    (((12, -1), (12, 0), (12, 1), (11, -1), (11, 0)), 3),
    (((1, -1), (1, 0), (1, 1), (14, -1), (14, 0), (14, 1), (13, 0)), 2),
    (((20, -1), (20, 0), (20, 1), (18, -1), (18, 0), (18, 1)), 10),
    (((21, -1), (21, 0), (21, 1), (17, -1), (17, 0), (17, 1)), 11),
    (((1, 1),), 1),
)
G1, G63, G64, G65, G128, G129, G3 = range(7)


class Layout:
    """the contig lengths of the seven reference genomes for one fragLen, and the bin arithmetic of the reducer over them"""

    def __init__(self, frag_len):
        self.frag_len, self.bin_w = frag_len, frag_len - 20
        self.genomes = []                               # contig lengths per genome
        for g, (big, tiny) in enumerate(SPEC):
            lens = [k * self.bin_w + d for k, d in big] + [TINY[(g + i) % len(TINY)] for i in range(tiny)]
            if g == G3:
                lens = lens[::-1]                       # the short contig first: the last contig of the set ends on k * binW + 1
            self.genomes.append(lens)
        self.genomes[G1] = [10]                         # a genome that is one contig shorter than a k-mer
        self.contig_len = np.array([n for lens in self.genomes for n in lens], dtype=np.int64)
        self.contig_genome = np.array([g for g, lens in enumerate(self.genomes) for _ in lens], dtype=np.int64)
        self.contig_bins = self.contig_len // self.bin_w + 1
        self.genome_contigs = [np.flatnonzero(self.contig_genome == g) for g in range(len(self.genomes))]
        self.n_contigs = len(self.contig_len)

    def bin_totals(self):
        return tuple(int(sum(n // self.bin_w + 1 for n in lens)) for lens in self.genomes)

    def sequences(self):
        return [[rng_genome(1000 * self.frag_len + 100 * g + c, n) for c, n in enumerate(lens)] for g, lens in enumerate(self.genomes)]

    def genome_bins(self, g):
        """(contig, bin inside the contig) of every bin of genome g, in the order k_pair_reduce adds them"""
        return [(int(c), j) for c in self.genome_contigs[g] for j in range(int(self.contig_bins[c]))]

    def pos_in_bin(self, c, j, r):
        """a start position of contig c inside its bin j"""
        lo, hi = j * self.bin_w, min((j + 1) * self.bin_w - 1, int(self.contig_len[c]))
        return int(r.integers(lo, hi + 1))


def check_layout(lay):
    """the edges the cases rely on, from the contig lengths alone"""
    assert lay.bin_totals() == BIN_TOTALS, lay.bin_totals()
    rest = {int(n) % lay.bin_w for n in lay.contig_len if n >= lay.bin_w}
    assert rest >= {lay.bin_w - 1, 0, 1}, rest           # lengths k * binW - 1, k * binW, k * binW + 1
    assert min(lay.contig_len) < K and lay.genomes[G1] == [10] and any(n < K for g in (G63, G129) for n in lay.genomes[g])
    assert all(len(lens) >= 2 for g, lens in enumerate(lay.genomes) if g != G1)
    assert lay.frag_len != 1000 or int(lay.contig_len.sum()) < 400000, int(lay.contig_len.sum())      # a sketch of seconds on the CPU stand-in


# ---- the reference set: one device sketch, one oracle sketch ----
_oracles = {}


class Ref:
    def __init__(self, engine, frag_len, ref_id_base=0):
        self.lay = Layout(frag_len)
        self.p = engine.params(K, frag_len)
        key = (frag_len, self.p.windowSize)
        if key not in _oracles:
            seqs = self.lay.sequences()
            _oracles[key] = (seqs, orc.Sketch(seqs, K, self.p.windowSize))
        seqs, self.osk = _oracles[key]
        self.engine = engine
        self.sk = Sketch(engine, self.p, seqs)
        st = self.sk.stats()
        assert st["contigs"] == self.lay.n_contigs and st["genomes"] == len(BIN_TOTALS)
        if ref_id_base:
            self.sk.set_ref_id_base(ref_id_base)

    def expected(self, maps, total, qid):
        return self.osk.compute_cgi(maps, total, qid, self.lay.frag_len)

    def close(self):
        self.sk.close()


def minimizer_count(frag_len, window):
    """minimizers of the layout's sketch (to choose ANI_MAX_INDEX_MINIMIZERS for a number of index chunks)"""
    lay = Layout(frag_len)
    return len(orc.Sketch(lay.sequences(), K, window).minimizers())


def same_rows(got, exp):
    """the whole record arrays, the identity as bits"""
    got, exp = np.ascontiguousarray(got, dtype=CGI_DT), np.ascontiguousarray(exp, dtype=CGI_DT)
    return got.shape == exp.shape and np.array_equal(got.view("<u4"), exp.view("<u4"))


# ---- mapping lists ----
def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def full_mantissa(r, n, lo=75.0, hi=100.0):
    """float32 identities in [lo, hi] with random low mantissa bits"""
    v = r.uniform(lo, hi, n).astype(np.float32)
    return np.minimum(v, np.float32(hi))


def mappings(lay, q, c, pos, ident):
    """a MAPPING_DT array; the reducer reads querySeqId, refSeqId, refStartPos and nucIdentity, the rest is filled as Map would"""
    m = np.zeros(len(q), dtype=MAPPING_DT)
    m["querySeqId"], m["refSeqId"], m["refStartPos"] = q, c, pos
    m["nucIdentity"] = np.asarray(ident, dtype=np.float32)
    m["queryLen"] = lay.frag_len
    m["refEndPos"] = m["refStartPos"] + lay.frag_len - 1
    m["queryEndPos"] = lay.frag_len - 1
    m["nucIdentityUpperBound"] = 100.0
    m["sketchSize"], m["conservedSketches"] = 80, 40
    return m


def list_random(lay, seed=1, n=None):
    """uniform contigs and positions, full-mantissa identities; -> (mappings, fragments)"""
    r = rng(11, lay.frag_len, seed)
    n = int(r.integers(1, 4001)) if n is None else n
    frags = max(1, n // 3)
    c = r.integers(0, lay.n_contigs, n)
    pos = (r.random(n) * (lay.contig_len[c] + 1)).astype(np.int64)
    return mappings(lay, r.integers(0, frags, n), c, pos, full_mantissa(r, n)), frags


def list_ties(lay, seed=1):
    """3 to 5 distinct identities: a fragment's mappings to one genome tie on the identity across contigs and, inside a contig, across
    positions, and the bins are few enough for the fragments to meet in them — another winner is another bin and another row"""
    r = rng(12, lay.frag_len, seed)
    values = full_mantissa(r, int(r.integers(3, 6)))
    n, frags = 4000, 250
    q = r.integers(0, frags, n)
    g = r.integers(1, len(BIN_TOTALS), n)
    c = np.array([r.choice(lay.genome_contigs[x]) for x in g])
    # a few start positions per contig, in different bins where the contig has several
    slots = (r.integers(0, 4, n) * lay.contig_len[c]) // 3
    pos = np.minimum(slots + r.integers(0, 2, n), lay.contig_len[c])
    return mappings(lay, q, c, pos, values[r.integers(0, len(values), n)]), frags


def list_bin_edges(lay, seed=1):
    """every contig: refStartPos 0, contigLen (the largest value accepted) and j * binW - 1, j * binW, j * binW + 1 for every j, each the
    only mapping of a fragment of its own"""
    r = rng(13, lay.frag_len, seed)
    c, pos = [], []
    for x in range(lay.n_contigs):
        n = int(lay.contig_len[x])
        here = {0, n}
        for j in range(1, n // lay.bin_w + 2):
            here |= {p for p in (j * lay.bin_w - 1, j * lay.bin_w, j * lay.bin_w + 1) if 0 <= p <= n}
        c += [x] * len(here)
        pos += sorted(here)
    n = len(c)
    return mappings(lay, r.permutation(n), c, pos, full_mantissa(r, n)), n


def list_dense(lay, seed=1):
    """every bin of the 129-bin and of the 65-bin genome occupied once, by fragments of their own"""
    r = rng(14, lay.frag_len, seed)
    c, pos = [], []
    for g in (G129, G65):
        for x, j in lay.genome_bins(g):
            c.append(x)
            pos.append(lay.pos_in_bin(x, j, r))
    n = len(c)
    return mappings(lay, r.permutation(n), c, pos, full_mantissa(r, n)), n


DENSE_SEED = 1


def dense_reverse_sums(lay, maps):
    """per genome of list_dense, the mean of its bins added in REVERSE bin order in float32: what a reducer that sums in another order
    than (contig, bin) ascending would report"""
    out = {}
    for g in (G129, G65):
        at = {(int(m["refSeqId"]), int(m["refStartPos"]) // lay.bin_w): m["nucIdentity"] for m in maps if lay.contig_genome[m["refSeqId"]] == g}
        bins = lay.genome_bins(g)
        assert sorted(at) == sorted(bins)
        s = np.float32(0.0)
        for b in reversed(bins):
            s = np.float32(s + at[b])
        out[g] = np.float32(s / np.float32(len(bins)))
    return out


def list_last_bin_only(lay, seed=1):
    """one mapping in the last bin of the last genome, one in bin 63 and one in bin 64 of the 65-bin genome"""
    r = rng(15, lay.frag_len, seed)
    last = lay.n_contigs - 1
    spots = [(last, int(lay.contig_len[last]))]
    bins = lay.genome_bins(G65)
    assert len(bins) == 65 and lay.contig_genome[last] == len(BIN_TOTALS) - 1
    spots += [(x, lay.pos_in_bin(x, j, r)) for x, j in (bins[63], bins[64])]
    return mappings(lay, [0, 1, 2], [s[0] for s in spots], [s[1] for s in spots], full_mantissa(r, 3)), 3


def list_hot_bin(lay, seed=1):
    """5000 fragments, one mapping each, all into one bin: they contend on its atomicMax"""
    r = rng(16, lay.frag_len, seed)
    x, j = lay.genome_bins(G129)[70]
    n = 5000
    pos = [lay.pos_in_bin(x, j, r) for _ in range(n)]
    return mappings(lay, r.permutation(n), [x] * n, pos, full_mantissa(r, n)), n


def list_long_group(lay, lead, seed=1):
    """`lead` fragments of one mapping each, then one fragment with 3000 mappings, all to the 128-bin genome: in (querySeqId, refSeqId)
    order the long group's head is candidate `lead` — with 255 the last lane of a 256-thread workgroup of k_oneway_bins, with 256 the
    first lane of the next — and the group spans twelve workgroups"""
    r = rng(17, lay.frag_len, seed, lead)
    n = lead + 3000
    assert (lead + 3000 - 1) // TPB - (lead + 1) // TPB + 1 == 12      # the workgroups behind the head's own lane
    q = np.concatenate([np.arange(lead), np.full(3000, lead)])
    c = r.choice(lay.genome_contigs[G128], n)
    pos = (r.random(n) * (lay.contig_len[c] + 1)).astype(np.int64)
    ident = full_mantissa(r, n)
    ident[lead + r.integers(0, 3000, 40)] = np.float32(99.5)       # the group's best identity several times: the tie-break decides
    return mappings(lay, q, c, pos, ident), lead + 1


def list_sparse_ids(lay, seed=1):
    """querySeqId values with gaps, 0 and 2^31 - 1 among them"""
    r = rng(18, lay.frag_len, seed)
    ids = np.unique(np.concatenate([[0, 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 16, 2 ** 24 + 1], r.integers(0, 2 ** 31, 300)]))
    n = 2000
    c = r.integers(0, lay.n_contigs, n)
    pos = (r.random(n) * (lay.contig_len[c] + 1)).astype(np.int64)
    q = ids[r.integers(0, len(ids), n)]
    q[:2] = (0, 2 ** 31 - 1)
    return mappings(lay, q, c, pos, full_mantissa(r, n)), len(np.unique(q))


def list_single(lay, seed=1):
    m, _ = list_random(lay, seed, n=7)
    return m[3:4].copy(), 1


def list_empty(lay, seed=1):
    return np.zeros(0, dtype=MAPPING_DT), 0


# name -> (builder, the totalQueryFragments to run it with, as offsets to its number of distinct fragments)
LISTS = {
    "random": (list_random, (0,)),
    "random2": (lambda lay: list_random(lay, 2), (0,)),
    "random3": (lambda lay: list_random(lay, 3, n=4000), (0,)),
    "ties": (list_ties, (0,)),
    "bin_edges": (list_bin_edges, (0,)),
    "dense": (lambda lay: list_dense(lay, DENSE_SEED), (0,)),
    "last_bin_only": (list_last_bin_only, (0,)),
    "hot_bin": (list_hot_bin, (0,)),
    "long_group_255": (lambda lay: list_long_group(lay, 255), (0,)),
    "long_group_256": (lambda lay: list_long_group(lay, 256), (0,)),
    "sparse_ids": (list_sparse_ids, (-100, 100)),       # totalQueryFragments smaller and larger than the number of distinct ids
    "n1": (list_single, (0,)),
    "n0": (list_empty, (0, 5)),
}
MANY_LISTS = ("random", "ties", "bin_edges", "dense")


def in_order(maps):
    """sorted by (querySeqId, refSeqId): the order ani_compute_cgi takes without sorting"""
    return maps[np.lexsort((maps["refSeqId"], maps["querySeqId"]))]


def is_ordered(maps):
    key = (maps["querySeqId"].astype(np.int64) << 32) | maps["refSeqId"].astype(np.int64)
    return bool(np.all(key[1:] >= key[:-1]))


def shuffled(maps, seed=5):
    """a fixed random permutation: the device sort path"""
    out = maps[rng(19, seed, len(maps)).permutation(len(maps))]
    if is_ordered(out):
        out = in_order(maps)[::-1].copy()              # a handful of mappings that the permutation left in order
    assert len(maps) < 2 or not is_ordered(out)
    return out


# ---- ani_compute_cgi ----
def case_list(ref, name, runs=1):
    """the list `name`, once in (querySeqId, refSeqId) order (the host's fast path) and once shuffled (the device sort), against the
    oracle"""
    lay = ref.lay
    build, totals = LISTS[name]
    maps, frags = build(lay)
    if name == "dense":
        # the case must be able to show a wrong summation order: adding the bins in reverse gives another float for some row
        exp = ref.expected(maps, frags, 0)
        rev = dense_reverse_sums(lay, maps)
        assert [int(g) for g in exp["refGenomeId"]] == [G65, G129] and list(exp["countSeq"]) == [65, 129]
        assert any(rev[int(row["refGenomeId"])].tobytes() != row["identity"].tobytes() for row in exp), "reseed list_dense: DENSE_SEED"
    if name.startswith("long_group"):
        lead = frags - 1
        o = in_order(maps)
        assert o["querySeqId"][lead] == lead and (lead == 0 or o["querySeqId"][lead - 1] == lead - 1) and lead % TPB in (TPB - 1, 0)
    for off in totals:
        total, qid = max(frags + off, 0), 3 + len(maps) % 5
        exp = ref.expected(maps, total, qid)
        assert len(maps) == 0 or len(exp) >= 1
        for order in (in_order, shuffled):
            sent = order(maps)
            assert order is shuffled or is_ordered(sent)
            for run in range(runs):
                got = ref.sk.compute_cgi(sent, total, qid)
                assert same_rows(got, exp), "%s, fragLen %d, %s, run %d:\n%r\n%r" % (name, lay.frag_len, order.__name__, run, got, exp)


def bad_mappings(lay):
    """(what, field, value): one field of one mapping of `random` that ani_compute_cgi must refuse"""
    f32 = np.float32
    return (
        ("refSeqId -1", "refSeqId", -1), ("refSeqId nContigs", "refSeqId", lay.n_contigs),
        ("refStartPos -1", "refStartPos", -1), ("refStartPos contigLen + 1", "refStartPos", "past"),
        ("identity 0", "nucIdentity", f32(0.0)), ("identity -0.0", "nucIdentity", f32(-0.0)), ("identity negative", "nucIdentity", f32(-80.0)),
        ("identity NaN", "nucIdentity", f32(np.nan)), ("identity +inf", "nucIdentity", f32(np.inf)),
        ("identity above 100", "nucIdentity", np.nextafter(f32(100.0), f32(np.inf))),
        ("querySeqId negative", "querySeqId", -1),
    )


def case_arguments(ref):
    """every bad mapping is ANI_ERR_ARG, wherever it stands in the list, and the context reduces `random` correctly afterwards;
    identity exactly 100 is accepted"""
    lay = ref.lay
    maps, frags = list_random(lay)
    maps = in_order(maps)
    exp = ref.expected(maps, frags, 2)
    assert same_rows(ref.sk.compute_cgi(maps, frags, 2), exp)
    for i, (what, field, value) in enumerate(bad_mappings(lay)):
        at = (0, len(maps) // 2, len(maps) - 1)[i % 3]
        bad = maps.copy()
        bad[field][at] = lay.contig_len[bad["refSeqId"][at]] + 1 if isinstance(value, str) else value
        for sent in (bad, bad[at:at + 1]):
            try:
                rows = ref.sk.compute_cgi(sent, frags, 2)
            except AniError as e:
                assert e.code == ERR_ARG, (what, e)
            else:
                raise AssertionError("%s: accepted, rows %r" % (what, rows))
        assert same_rows(ref.sk.compute_cgi(maps, frags, 2), exp), "after " + what
    # a NaN must not get as far as displacing a valid identity of its bin: the pair is refused as a whole
    pair = maps[:2].copy()
    pair["querySeqId"], pair["refSeqId"], pair["refStartPos"] = (0, 1), pair["refSeqId"][0], pair["refStartPos"][0]
    pair["nucIdentity"] = (np.float32(90.0), np.float32(np.nan))
    try:
        ref.sk.compute_cgi(pair, 2, 0)
    except AniError as e:
        assert e.code == ERR_ARG
    else:
        raise AssertionError("a NaN identity beside a valid one was accepted")
    top = maps.copy()
    top["nucIdentity"][::7] = np.float32(100.0)
    assert same_rows(ref.sk.compute_cgi(top, frags, 2), ref.expected(top, frags, 2))
    past = maps.copy()
    past["refStartPos"] = lay.contig_len[past["refSeqId"]]            # contigLen itself is the largest value accepted
    assert same_rows(ref.sk.compute_cgi(past, frags, 2), ref.expected(past, frags, 2))


# ---- ani_reduce_check: several queries in one table ----
def bind(lib):
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.ani_reduce_check.argtypes = [vp, vp, vp, ctypes.c_size_t, vp, i32, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.ani_reduce_check.restype = ctypes.c_int
    return lib


def reduce_check(ref, maps, frag_start, genome_base, first_id):
    e = ref.engine
    lib = bind(e.lib)
    maps = np.ascontiguousarray(maps, dtype=MAPPING_DT)
    frag_start = np.ascontiguousarray(frag_start, dtype=np.int32)
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    e._chk(lib.ani_reduce_check(e.h, ref.sk.h, maps.ctypes.data if len(maps) else None, len(maps), frag_start.ctypes.data, len(frag_start) - 1,
                                genome_base, first_id, ctypes.byref(p), ctypes.byref(n)))
    return e._take(p, n.value, CGI_DT)


def split_queries(frags, n_query, seed):
    """queryFragStart: `frags` fragment ids cut into n_query non-empty queries"""
    cuts = np.sort(rng(20, seed, frags, n_query).choice(np.arange(1, frags), n_query - 1, replace=False)) if n_query > 1 else []
    return [0] + [int(c) for c in cuts] + [frags]


def with_empty(maps, start, first, last):
    """a query without mappings in front (`first` fragments: its ids are put in front of all others) and / or behind (`last` fragments);
    None: no such query, 0: a query of no fragments at all"""
    maps = maps.copy()
    if first is not None:
        maps["querySeqId"] += first
        start = [0] + [x + first for x in start]
    if last is not None:
        start = start + [start[-1] + last]
    return maps, start


def expected_many(ref, maps, frag_start, first_id):
    """the definition: ani_compute_cgi per query, by the oracle"""
    rows = []
    for q in range(len(frag_start) - 1):
        mine = maps[(maps["querySeqId"] >= frag_start[q]) & (maps["querySeqId"] < frag_start[q + 1])]
        rows.append(ref.expected(mine, frag_start[q + 1] - frag_start[q], first_id + q))
    return np.concatenate(rows) if rows else np.zeros(0, dtype=CGI_DT)


def case_many(ref, name):
    """the list `name` with its fragments spread over 1, 2 and 5 queries of one table (with 7 reference genomes 5 queries are 35
    pairs: the last workgroup of four waves of k_pair_reduce is partial), genomeBase 0 and 1000; and with a query without mappings in
    front and / or behind, of some fragments or of none: it gets no rows and the others keep theirs"""
    maps0, frags = LISTS[name][0](ref.lay)
    for n_query in (1, 2, 5):
        for genome_base in (0, 1000):
            for first, last in ((None, None), (7, None), (None, 9), (0, 0), (3, 0)):
                if (first, last) != (None, None) and (n_query, genome_base) not in ((2, 1000), (5, 0)):
                    continue
                maps, start = with_empty(maps0, split_queries(frags, n_query, n_query), first, last)
                first_id = 40 + n_query
                exp = expected_many(ref, maps, start, first_id)
                lead = 0 if first is None else 1
                ids = set(int(x) for x in exp["qryGenomeId"])
                assert ids == set(range(first_id + lead, first_id + lead + n_query)), (name, ids)       # the queries without mappings get no rows
                for order in (in_order, shuffled):
                    got = reduce_check(ref, order(maps), start, genome_base, first_id)
                    assert same_rows(got, exp), "%s, fragLen %d, %d queries %r, genomeBase %d, %s:\n%r\n%r" % (
                        name, ref.lay.frag_len, n_query, start, genome_base, order.__name__, got, exp)


def case_many_arguments(ref):
    """ani_reduce_check validates like ani_compute_cgi, refuses a querySeqId outside the table and a table that is not ascending, and
    works afterwards"""
    maps, frags = list_random(ref.lay)
    start = split_queries(frags, 2, 1)
    exp = expected_many(ref, maps, start, 0)
    nan = maps.copy()
    nan["nucIdentity"][1] = np.nan
    outside = maps.copy()
    outside["querySeqId"][len(maps) // 2] = frags
    for what, m, s in (("NaN", nan, start), ("querySeqId outside the table", outside, start), ("descending table", maps, [0, frags, frags - 1]),
                       ("table from 1", maps, [1, frags])):
        try:
            rows = reduce_check(ref, m, s, 0, 0)
        except AniError as e:
            assert e.code == ERR_ARG, (what, e)
        else:
            raise AssertionError("%s: accepted, rows %r" % (what, rows))
        assert same_rows(reduce_check(ref, maps, start, 0, 0), exp), "after " + what
    assert len(reduce_check(ref, maps[:0], [0], 0, 0)) == 0 and len(reduce_check(ref, maps[:0], [0, 0, 7], 5, 0)) == 0
