"""Host-side mirror of the reference seams over the C-ABI (include/ani_abi.h), via ctypes.

    Sketch(engine, params, genomes)        ≙ skch::Sketch::Sketch          (src/map/include/winSketch.hpp:109)
    Sketch.map_query(genome)               ≙ skch::Map::Map + callback     (src/map/include/computeMap.hpp:93)
    Sketch.compute_cgi(maps, total, qid)   ≙ cgi::computeCGI               (src/cgi/include/computeCoreIdentity.hpp:166)
    Sketch.map_cgi_batch(genomes, first)   ≙ the query loop of src/cgi/core_genome_identity.cpp:81-106
    Engine.cluster_greedy(rows, n, t)      greedy species clustering of the rows at an ANI threshold (no reference counterpart)
    Engine.tree_average(rows, n)           average-linkage (UPGMA) tree of the genomes, scipy linkage form (no reference counterpart)
    Engine.tree_nj(rows, n)                neighbour-joining tree of the genomes: children and branch lengths (no reference counterpart)
    Engine.tree_single(rows, n)            single-linkage tree of the genomes (scipy linkage form) and, with return_edges, its minimum
                                           spanning tree; memory follows the rows, no genome ceiling (no reference counterpart)
    Sketch.signatures(size)                bottom-`size` signatures of the reference genomes from their minimizers (no reference counterpart)
    Engine.signature_pairs(sig, len, k)    Mash-style ANI estimate between all pairs of signatures (no reference counterpart)
    Engine.tree_single_sketch(rows, n, sig, len, k)  tree_single with that estimate for every pair without rows, streamed strip by
                                           strip: nothing of size n^2 anywhere, no genome ceiling (no reference counterpart)
    Engine.signature_screen(ref, len, qry, len, k_mer, k)  the k nearest references of every query under that estimate
    Engine.signature_screen_contain(ref, len, qry, len, k_mer, k, mode)  the same under the containment estimate: partial genomes,
                                           plasmids and contigs against whole references, or references inside a larger assembly
    Engine.signature_neighbors(sig, len, k_mer, k)  the k nearest neighbours of every genome under that estimate, streamed strip by
                                           strip, no genome ceiling (no reference counterpart)
    Engine.signature_graph(sig, len, k_mer, t)  the pairs at or above the threshold t under that estimate or the symmetric containment
                                           estimate, filtered on the device strip by strip, no genome ceiling
    Engine.signature_cluster(sig, len, k_mer, t)  greedy representative clustering (dereplication) of the genomes under that estimate
                                           at the threshold t: genomes against representatives only, no genome ceiling
    Engine.signature_cluster_contain(sig, len, k_mer, t)  the same under the symmetric containment estimate: partial genomes (MAGs of
                                           unequal completeness) join the genome they are parts of

Everything here is plumbing: numpy arrays in, numpy record arrays out.  All compute happens in
libfastani_amd.so (hand-written HIP kernels, gfx950); there is no Python or CPU fallback.
"""
import ctypes as C
import weakref

import numpy as np

MINIMIZER_DT = np.dtype([("hash", "<u4"), ("seqId", "<i4"), ("wpos", "<i4")])
MAPPING_DT = np.dtype([("queryLen", "<i4"), ("refStartPos", "<i4"), ("refEndPos", "<i4"), ("queryStartPos", "<i4"),
                       ("queryEndPos", "<i4"), ("refSeqId", "<i4"), ("querySeqId", "<i4"), ("nucIdentity", "<f4"),
                       ("nucIdentityUpperBound", "<f4"), ("sketchSize", "<i4"), ("conservedSketches", "<i4")])
CGI_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("countSeq", "<i4"),
                   ("totalQueryFragments", "<i4"), ("identity", "<f4")])
SIGPAIR_DT = np.dtype([("a", "<i4"), ("b", "<i4"), ("shared", "<i4"), ("size", "<i4"), ("identity", "<f4")])
NEIGHBOR_DT = np.dtype([("neighbor", "<i4"), ("shared", "<i4"), ("size", "<i4"), ("identity", "<f4")])
BINPROFILE_DT = np.dtype([("count", "<u4"), ("minIdentity", "<f4"), ("maxIdentity", "<f4"), ("reserved", "<u4"), ("sum", "<u8")])
FRAGDIST_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("count", "<u4"), ("minIdentity", "<f4"), ("q1", "<f4"), ("median", "<f4"),
                        ("q3", "<f4"), ("maxIdentity", "<f4"), ("sum", "<u8")])
HIT_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("refSeqId", "<i4"), ("refStartPos", "<i4"), ("querySeqId", "<i4"), ("identity", "<f4")])
CI_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("count", "<u4"), ("replicates", "<u4"), ("sum", "<u8"), ("lowSum", "<u8"),
                  ("highSum", "<u8"), ("low", "<f4"), ("high", "<f4")])
BOOT_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("count", "<u4"), ("replicates", "<u4"), ("sum", "<u8")])
TREE_METHODS = {"average": 0, "nj": 1, "single": 2}          # ANI_TREE_AVERAGE, ANI_TREE_NJ, ANI_TREE_SINGLE
PAINT_DT = np.dtype([("qryGenomeId", "<i4"), ("querySeqId", "<i4"), ("refGenomeId", "<i4"), ("refSeqId", "<i4"), ("refStartPos", "<i4"), ("identity", "<f4"),
                     ("secondGenomeId", "<i4"), ("secondIdentity", "<f4"), ("genomes", "<u4"), ("reserved", "<u4")])
SYNTENY_DT = np.dtype([("refGenomeId", "<i4"), ("qryGenomeId", "<i4"), ("count", "<u4"), ("forward", "<u4"), ("reverse", "<u4"), ("breaks", "<u4"),
                       ("contigBorders", "<u4"), ("blocks", "<u4"), ("reverseBlocks", "<u4"), ("reverseHits", "<u4"), ("largestBlock", "<u4"),
                       ("singletons", "<u4")])
SYNBLOCK_DT = np.dtype([("refSeqId", "<i4"), ("refStartFirst", "<i4"), ("refStartLast", "<i4"), ("qSeqFirst", "<i4"), ("qSeqLast", "<i4"),
                        ("hits", "<u4"), ("idSum", "<u8")])

ANI_SEQ_HOST_ASCII = 0
ANI_SEQ_DEVICE_PACKED2 = 1
ANI_SEQ_HOST_ASCII_PTRS = 2
ANI_SEQ_DEVICE_BATCH = 3
ANI_SEQ_HOST_MIXED_PTRS = 4


class AniError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ani error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("kmerSize", C.c_int32), ("windowSize", C.c_int32), ("fragLen", C.c_int32),
                ("percentageIdentity", C.c_float)]


class SeqBatch(C.Structure):
    _fields_ = [("layout", C.c_int32), ("nGenomes", C.c_int32), ("nContigs", C.c_int32),
                ("genomeContigStart", C.c_void_p), ("contigOffset", C.c_void_p), ("contigLen", C.c_void_p),
                ("data", C.c_void_p)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("refBases", "refMinimizers", "refUniqueHashes", "queryGenomes", "queryFragments",
                                          "queryBases", "querySketchHashes", "seedHits", "l1Candidates", "l2WindowEntries",
                                          "l2Steps", "l2QueryHashes", "l2WindowEntriesB", "l2QueryHashesB", "l2Launches", "l2FastCandidates", "l2SlowCandidates", "l2SlowLimit", "l2SlowDup", "l2SlowOverflow", "mappings", "cgiRows", "indexChunks", "l1Probes", "l2ChunkHalvings", "indexChunkBuilds", "l1BigFragments", "l1MidFragments", "l1TinyFragments")] + \
               [(n, C.c_double) for n in ("msSketch", "msIndex", "msFragSketch", "msL1", "msL2", "msReduce", "msL2Kernel", "msL2Ranges", "msL2Codes", "msL2Slow", "msL2SimB", "msL1Probe", "msL1Main", "msL1Big", "msL1Tiny")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _bind(lib):
    vp = C.c_void_p
    sig = {
        "ani_init": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "ani_shutdown": (None, [vp]),
        "ani_last_error": (C.c_char_p, []),
        "ani_free": (None, [vp]),
        "ani_device_free": (None, [vp, vp]),
        "ani_device_copy": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ani_device_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        "ani_device_copy_peer": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "ani_pack_acgt": (C.c_int, [vp, C.c_int32, vp]),
        "ani_batch_upload": (C.c_int, [vp, C.POINTER(SeqBatch), C.POINTER(vp)]),
        "ani_batch_free": (None, [vp]),
        "ani_get_counters": (C.c_int, [vp, C.POINTER(Counters)]),
        "ani_reset_counters": (C.c_int, [vp]),
        "ani_params_default": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int]),
        "ani_recommended_window": (C.c_int, [C.c_int, C.c_int]),
        "ani_min_hits_relaxed": (C.c_int, [C.c_int, C.c_int, C.c_float]),
        "ani_identity": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "ani_sketch_build": (C.c_int, [vp, C.POINTER(Params), C.POINTER(SeqBatch), C.POINTER(vp)]),
        "ani_sketch_destroy": (None, [vp]),
        "ani_sketch_export": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_stats": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "ani_sketch_chunks": (C.c_int, [vp, C.POINTER(C.c_int32), vp, C.c_int32]),
        "ani_sketch_records": (C.c_int, [vp, C.POINTER(Params), C.POINTER(SeqBatch), C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_from_records": (C.c_int, [vp, C.POINTER(Params), vp, C.c_size_t, vp, C.c_int32, vp, C.c_int32, C.POINTER(vp)]),
        "ani_sketch_from_record_parts": (C.c_int, [vp, C.POINTER(Params), C.c_int32, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.POINTER(vp)]),
        "ani_sketch_adopt_record_parts": (C.c_int, [vp, C.POINTER(Params), C.c_int32, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.POINTER(vp)]),
        "ani_map_query": (C.c_int, [vp, vp, C.POINTER(SeqBatch), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
        "ani_query_sketch": (C.c_int, [vp, C.POINTER(Params), C.POINTER(SeqBatch), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_compute_cgi": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint64, C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_save": (C.c_int, [vp, C.c_char_p, vp]),
        "ani_sketch_load": (C.c_int, [vp, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(vp)]),
        "ani_sketch_writer_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "ani_sketch_writer_add": (C.c_int, [vp, vp, vp]),
        "ani_sketch_writer_close": (C.c_int, [vp]),
        "ani_sketch_writer_abort": (None, [vp]),
        "ani_device_memory": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ani_pool_prewarm_index": (C.c_int, [vp, C.c_uint64]),
        "ani_pool_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "ani_sketch_file_info": (C.c_int, [C.c_char_p, C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
        "ani_sketch_genome_name": (C.c_char_p, [vp, C.c_int32]),
        "ani_sketch_tables": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "ani_fragset_build": (C.c_int, [vp, C.POINTER(Params), C.POINTER(SeqBatch), C.POINTER(vp)]),
        "ani_sketch_records_self": (C.c_int, [vp, C.POINTER(Params), C.POINTER(SeqBatch), C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]),
        "ani_map_cgi_fragset": (C.c_int, [vp, vp, vp, C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_fragset_free": (None, [vp]),
        "ani_map_cgi_fragsets": (C.c_int, [vp, vp, C.c_int32, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_fragset_info": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]),
        "ani_fragset_pack_bytes": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
        "ani_fragset_pack": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "ani_fragset_unpack": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(vp)]),
        "ani_fragset_unpack_merged": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, vp, C.POINTER(vp)]),
        "ani_sketch_residency": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "ani_sketch_set_ref_id_base": (C.c_int, [vp, C.c_int32]),
        "ani_map_cgi_batch": (C.c_int, [vp, vp, C.POINTER(SeqBatch), C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_profile_begin": (C.c_int, [vp, C.c_float, C.c_int32]),
        "ani_sketch_profile_bins": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "ani_sketch_profile_read": (C.c_int, [vp, vp, vp]),
        "ani_sketch_profile_end": (C.c_int, [vp]),
        "ani_sketch_fragdist_begin": (C.c_int, [vp, C.c_float, C.c_int32, vp, C.c_int32]),
        "ani_sketch_fragdist_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_fragdist_end": (C.c_int, [vp]),
        "ani_sketch_hits_begin": (C.c_int, [vp, C.c_float, C.c_int32]),
        "ani_sketch_hits_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_hits_end": (C.c_int, [vp]),
        "ani_sketch_ci_begin": (C.c_int, [vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]),
        "ani_sketch_ci_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_ci_end": (C.c_int, [vp]),
        "ani_sketch_boot_begin": (C.c_int, [vp, C.c_float, C.c_int32, C.c_int32, C.c_uint32]),
        "ani_sketch_boot_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_boot_end": (C.c_int, [vp]),
        "ani_tree_support": (C.c_int, [vp, C.c_int32, vp, C.c_int32, C.c_int32, vp]),
        "ani_tree_support_bootstrap": (C.c_int, [vp, C.c_int32, vp, C.c_size_t, C.c_int32, C.c_float, vp, C.c_int32, vp, vp]),
        "ani_sketch_paint_begin": (C.c_int, [vp]),
        "ani_sketch_paint_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_paint_end": (C.c_int, [vp]),
        "ani_sketch_synteny_begin": (C.c_int, [vp, C.c_float, C.c_int32]),
        "ani_sketch_synteny_take": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_sketch_synteny_end": (C.c_int, [vp]),
        "ani_paint_merge": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ani_synth_packed": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, vp]),
        "ani_synth_packed_clusters": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]),
        "ani_cluster_greedy": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, C.c_float, vp, vp]),
        "ani_tree_average": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, C.c_float, vp, vp]),
        "ani_tree_nj": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, C.c_float, vp, vp]),
        "ani_tree_single": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, C.c_float, vp, vp, vp]),
        "ani_tree_single_rounds": (C.c_int, [vp]),
        "ani_tree_single_sketch": (C.c_int, [vp, vp, C.c_size_t, C.c_int32, C.c_float, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]),
        "ani_tree_single_sketch_strips": (C.c_int, [vp, vp, C.c_size_t]),
        "ani_sketch_signatures": (C.c_int, [vp, C.c_int32, vp, vp]),
        "ani_signature_pairs": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
        "ani_signature_neighbors": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
        "ani_signature_neighbors_strips": (C.c_int, [vp]),
        "ani_signature_graph": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
        "ani_signature_graph_strips": (C.c_int, [vp]),
        "ani_signature_screen": (C.c_int, [vp, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, vp, vp]),
        "ani_signature_screen_contain": (C.c_int, [vp, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                                   vp, vp]),
        "ani_signature_screen_strips": (C.c_int, [vp]),
        "ani_signature_screen_tile": (None, [vp, vp, vp]),
        "ani_signature_cluster": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, vp, vp]),
        "ani_signature_cluster_contain": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, vp, vp]),
        "ani_signature_cluster_stats": (C.c_int, [vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sorted(sig)


ABI_SYMBOLS = None


class HostGenomes:
    """A batch of genomes in host memory: list of genomes, each a list of contigs (bytes / str / uint8 arrays).
    Bytes are passed as read from FASTA; the library upper-cases them (commonFunc.hpp:56-66)."""

    def __init__(self, genomes):
        self.contig_start = [0]
        lens, offs, parts = [], [], []
        off = 0
        for contigs in genomes:
            for c in contigs:
                if isinstance(c, str):
                    c = c.encode()
                a = np.frombuffer(bytes(c), dtype=np.uint8) if isinstance(c, (bytes, bytearray)) else np.ascontiguousarray(c, dtype=np.uint8)
                parts.append(a)
                lens.append(len(a))
                offs.append(off)
                off += len(a)
            self.contig_start.append(len(lens))
        self.data = np.concatenate(parts) if parts else np.zeros(1, dtype=np.uint8)
        if len(self.data) == 0:
            self.data = np.zeros(1, dtype=np.uint8)
        self.gcs = np.asarray(self.contig_start, dtype=np.int32)
        self.off = np.asarray(offs if offs else [0], dtype=np.int64)
        self.len = np.asarray(lens if lens else [0], dtype=np.int32)
        self.n_genomes = len(genomes)
        self.n_contigs = len(lens)

    def batch(self):
        b = SeqBatch()
        b.layout = ANI_SEQ_HOST_ASCII
        b.nGenomes = self.n_genomes
        b.nContigs = self.n_contigs
        b.genomeContigStart = self.gcs.ctypes.data
        b.contigOffset = self.off.ctypes.data
        b.contigLen = self.len.ctypes.data
        b.data = self.data.ctypes.data
        return b


class DeviceGenomes:
    """Single-contig genomes of equal length, 2-bit packed, already resident in device memory at `dev_ptr`
    (genome i at word offset i*ceil(len/16)) — the synthetic benchmark input."""

    def __init__(self, dev_ptr, n_genomes, genome_len, first=0, count=None):
        count = n_genomes - first if count is None else count
        words = (genome_len + 15) // 16
        self.gcs = np.arange(count + 1, dtype=np.int32)
        self.off = (np.arange(first, first + count, dtype=np.int64) * words)
        self.len = np.full(count, genome_len, dtype=np.int32)
        self.dev_ptr = dev_ptr
        self.n_genomes = count
        self.n_contigs = count

    def batch(self):
        b = SeqBatch()
        b.layout = ANI_SEQ_DEVICE_PACKED2
        b.nGenomes = self.n_genomes
        b.nContigs = self.n_contigs
        b.genomeContigStart = self.gcs.ctypes.data
        b.contigOffset = self.off.ctypes.data
        b.contigLen = self.len.ctypes.data
        b.data = self.dev_ptr
        return b


class UploadedGenomes:
    """Host genomes packed and copied to the device once (ani_batch_upload); usable as references and as queries."""

    def __init__(self, engine, genomes, ptrs=False, mixed=False):
        self.e = engine
        self.host = genomes if isinstance(genomes, HostGenomes) else HostGenomes(genomes)
        b = self.host.batch()
        if ptrs or mixed:                          # per-contig pointer layout (ANI_SEQ_HOST_ASCII_PTRS)
            self._ptrs = (self.host.data.ctypes.data + self.host.off[:max(self.host.n_contigs, 1)]).astype(np.uint64)
            b.layout = ANI_SEQ_HOST_ASCII_PTRS
            b.data = self._ptrs.ctypes.data
            b.contigOffset = None
        if mixed:                                  # ANI_SEQ_HOST_MIXED_PTRS: every contig that ani_pack_acgt accepts goes over as 2-bit codes
            nc = self.host.n_contigs
            self._kind = np.zeros(max(nc, 1), dtype=np.int64)
            self._packed = []
            for c in range(nc):
                ln = int(self.host.len[c])
                out = np.zeros((ln + 15) // 16 + 2, dtype=np.uint32)
                if engine.lib.ani_pack_acgt(C.c_void_p(int(self._ptrs[c])), ln, out.ctypes.data_as(C.c_void_p)) == 1:
                    self._kind[c] = 1
                    self._packed.append(out)
                    self._ptrs[c] = out.ctypes.data
            b.layout = ANI_SEQ_HOST_MIXED_PTRS
            b.contigOffset = self._kind.ctypes.data
            self.packed_contigs = int(self._kind[:nc].sum())
        h = C.c_void_p()
        engine._chk(engine.lib.ani_batch_upload(engine.h, C.byref(b), C.byref(h)))
        self.h = h
        self.n_genomes = self.host.n_genomes
        self.n_contigs = self.host.n_contigs

    def batch(self):
        b = self.host.batch()
        b.layout = ANI_SEQ_DEVICE_BATCH
        b.data = self.h
        return b

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.ani_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def paint_merge(a, b, lib=None):
    """-> PAINT_DT[n]: the records of two lists over disjoint sets of reference genomes, each in (qryGenomeId, querySeqId) order, joined
    into the list over the union (ani_paint_merge: a host function, no engine).  `lib`: the library to call, the product library by
    default."""
    if lib is None:
        from . import _lib
        lib = _lib.load()
    if lib.ani_paint_merge.argtypes is None:      # no Engine has bound this library yet
        _bind(lib)
    a, b = np.ascontiguousarray(a, dtype=PAINT_DT), np.ascontiguousarray(b, dtype=PAINT_DT)
    rp, n = C.c_void_p(), C.c_size_t()
    rc = lib.ani_paint_merge(a.ctypes.data if len(a) else None, len(a), b.ctypes.data if len(b) else None, len(b), C.byref(rp), C.byref(n))
    if rc != 0:
        raise AniError(rc, (lib.ani_last_error() or b"").decode())
    if n.value == 0 or not rp.value:
        lib.ani_free(rp)
        return np.zeros(0, dtype=PAINT_DT)
    return np.asarray(_OwnedBuffer(lib, rp.value, n.value, PAINT_DT))


def boot_identity(records, sums):
    """-> float32[n, B]: the replicate identities of the records and sums of Sketch.boot_take, by the boot records' rule 3 of ani_abi.h:
    (float)((double) S[r] / ((double) count * 1048576.0))"""
    records = np.ascontiguousarray(records, dtype=BOOT_DT)
    sums = np.ascontiguousarray(sums, dtype=np.uint64).reshape(len(records), -1)
    return (sums.astype(np.float64) / (records["count"].astype(np.float64) * 1048576.0)[:, None]).astype(np.float32)


def tree_support(children, rep_children, unrooted=False, lib=None):
    """-> uint32[n_genomes - 1]: per record of the tree `children` (int (n_genomes - 1, 2), the record form of Engine.tree_average /
    tree_single (columns 0 and 1 of the linkage) / tree_nj) the number of replicate trees `rep_children` (int (B, n_genomes - 1, 2)) that
    hold the same clade — with `unrooted` the same split (ani_tree_support: a host function, no engine).  `lib`: the library to call,
    the product library by default."""
    if lib is None:
        from . import _lib
        lib = _lib.load()
    if lib.ani_tree_support.argtypes is None:      # no Engine has bound this library yet
        _bind(lib)
    children = np.ascontiguousarray(np.asarray(children).reshape(-1, 2), dtype=np.int32)
    m = len(children)
    rep_children = np.ascontiguousarray(np.asarray(rep_children).reshape(-1, m, 2) if m else np.zeros((0, 0, 2)), dtype=np.int32)
    support = np.zeros(m, dtype=np.uint32)
    rc = lib.ani_tree_support(children.ctypes.data if m else None, m + 1, rep_children.ctypes.data if rep_children.size else None,
                              len(rep_children), 1 if unrooted else 0, support.ctypes.data if m else None)
    if rc != 0:
        raise AniError(rc, (lib.ani_last_error() or b"").decode())
    return support


def _as_batch(g):
    if isinstance(g, (HostGenomes, DeviceGenomes, UploadedGenomes)):
        return g
    return HostGenomes(g)


class _OwnedBuffer:
    """a buffer the library allocated (ani_free releases it), exposed through the array interface"""

    def __init__(self, lib, address, n, dt):
        self._lib, self._address = lib, address
        self.__array_interface__ = dict(shape=(n,), typestr=dt.str, descr=dt.descr, data=(address, False), version=3)

    def __del__(self):
        try:
            self._lib.ani_free(C.c_void_p(self._address))
        except Exception:                       # interpreter shutdown: the process frees it
            pass


class Engine:
    """One ani_ctx: one device, one host thread."""

    def __init__(self, lib, device=0):
        global ABI_SYMBOLS
        self.lib = lib
        ABI_SYMBOLS = _bind(lib)
        h = C.c_void_p()
        self._chk(lib.ani_init(device, C.byref(h)))
        self.h = h
        self._sketches = weakref.WeakSet()      # live sketches are destroyed before the context (see close)

    def _chk(self, rc):
        if rc != 0:
            raise AniError(rc, (self.lib.ani_last_error() or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            for sk in list(self._sketches):
                sk.close()
            self.lib.ani_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self, k=16, frag_len=3000):
        p = Params()
        self._chk(self.lib.ani_params_default(C.byref(p), k, frag_len))
        return p

    def counters(self):
        c = Counters()
        self._chk(self.lib.ani_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        self._chk(self.lib.ani_reset_counters(self.h))

    def _take(self, ptr, n, dt):
        """the library's malloc'ed result buffer as a numpy array WITHOUT a copy: the array (and every view of it) keeps an owner
        object alive that hands the buffer to ani_free when the last of them is gone.  (A copy of the 785 k result rows of the
        1000 x 1000 job into a fresh array was 2 - 3 ms of page faults and memmove per step.)"""
        if n == 0 or not ptr.value:
            self.lib.ani_free(ptr)
            return np.zeros(0, dtype=dt)
        return np.asarray(_OwnedBuffer(self.lib, ptr.value, n, np.dtype(dt)))

    def query_sketch(self, params, genomes):
        g = _as_batch(genomes)
        b = g.batch()
        hp, op, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._chk(self.lib.ani_query_sketch(self.h, C.byref(params), C.byref(b), C.byref(hp), C.byref(op), C.byref(n)))
        offs = self._take(op, n.value + 1, np.dtype("<u8"))
        hashes = self._take(hp, int(offs[-1]), np.dtype("<u4"))
        return [hashes[int(offs[i]):int(offs[i + 1])] for i in range(n.value)]

    def synth_packed(self, seed, first_genome, n_genomes, genome_len, dev_ptr, variant=0, cluster_size=20):
        self._chk(self.lib.ani_synth_packed_clusters(self.h, seed, variant, first_genome, n_genomes, genome_len, cluster_size, dev_ptr))

    def sketch_records(self, params, genomes, seq_id_base):
        """-> (device pointer to 12-byte records, count); free with device_free."""
        g = _as_batch(genomes)
        b = g.batch()
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.ani_sketch_records(self.h, C.byref(params), C.byref(b), seq_id_base, C.byref(p), C.byref(n)))
        return p.value, n.value

    def sketch_records_self(self, params, genomes, seq_id_base):
        """all-vs-all: -> (device pointer to 12-byte records, count, FragmentSet of the same genomes)"""
        g = _as_batch(genomes)
        b = g.batch()
        p, n, f = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self._chk(self.lib.ani_sketch_records_self(self.h, C.byref(params), C.byref(b), seq_id_base, C.byref(p), C.byref(n), C.byref(f)))
        return p.value, n.value, FragmentSet(self, f)

    def fragment_set(self, params, genomes):
        g = _as_batch(genomes)
        b = g.batch()
        f = C.c_void_p()
        self._chk(self.lib.ani_fragset_build(self.h, C.byref(params), C.byref(b), C.byref(f)))
        return FragmentSet(self, f)

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.ani_device_alloc(self.h, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, ptr):
        self.lib.ani_device_free(self.h, ptr)

    def pool_prewarm_index(self, n_minimizers):
        """a hint (ani_abi.h): the device memory sketching and indexing about n_minimizers minimizers will take, reserved now"""
        self._chk(self.lib.ani_pool_prewarm_index(self.h, int(n_minimizers)))

    def pool_stats(self):
        """the device allocator (ani_pool_stats): segment / free / live bytes, segments, hipMalloc calls / bytes / microseconds so far"""
        out = (C.c_uint64 * 8)()
        self._chk(self.lib.ani_pool_stats(self.h, out))
        keys = ("segment_bytes", "free_bytes", "live_bytes", "segments", "hipmalloc_calls", "hipmalloc_bytes", "hipmalloc_us", "largest_free_extent")
        return dict(zip(keys, [int(x) for x in out]))

    def device_copy(self, dst, src, nbytes):
        self._chk(self.lib.ani_device_copy(self.h, dst, src, nbytes))

    def cluster_greedy(self, rows, n_genomes, min_identity):
        """greedy clustering of the pair graph w(i, j) >= min_identity (ani_cluster_greedy): `rows` a CGI_DT array whose qryGenomeId /
        refGenomeId are ids in one numbering [0, n_genomes); the rows of a pair are folded in the order given, self rows ignored.
        -> (representative int32[n_genomes], identity float32[n_genomes]); a representative is its own, with identity 0."""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        n_genomes = int(n_genomes)
        rep = np.empty(max(n_genomes, 0), dtype=np.int32)
        ident = np.empty(max(n_genomes, 0), dtype=np.float32)
        self._chk(self.lib.ani_cluster_greedy(self.h, rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(min_identity),
                                              rep.ctypes.data if n_genomes > 0 else None, ident.ctypes.data if n_genomes > 0 else None))
        return rep, ident

    def tree_average(self, rows, n_genomes, missing_identity=0.0):
        """average-linkage (UPGMA) tree of the genomes over the pair distances 1 - w / 100 (ani_tree_average): `rows` as for
        cluster_greedy, a pair without rows at 1 - missing_identity / 100.  -> scipy linkage matrix, float64 (n_genomes - 1, 4): child,
        child (smaller id first), height, leaf count; (0, 4) for n_genomes <= 1."""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        n_genomes = int(n_genomes)
        m = max(n_genomes - 1, 0)
        children = np.empty(2 * m, dtype=np.int32)
        height = np.empty(m, dtype=np.float32)
        self._chk(self.lib.ani_tree_average(self.h, rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(missing_identity),
                                            children.ctypes.data if m else None, height.ctypes.data if m else None))
        z = np.empty((m, 4), dtype=np.float64)
        z[:, 0:2] = children.reshape(m, 2)
        z[:, 2] = height
        count = np.ones(n_genomes + m, dtype=np.int64)
        for s, (x, y) in enumerate(children.reshape(m, 2).tolist()):
            count[n_genomes + s] = count[x] + count[y]
        z[:, 3] = count[n_genomes:]
        return z

    def tree_nj(self, rows, n_genomes, missing_identity=0.0):
        """neighbour-joining tree of the genomes over the fixed-point pair distances (ani_tree_nj; the semantics are in ani_abi.h):
        `rows` as for cluster_greedy, a pair without rows at missing_identity.  -> (children int64 (n_genomes - 1, 2), lengths float32
        (n_genomes - 1, 2)): record s joins the nodes children[s] (smaller id first; a leaf's id is its index, join s makes node
        n_genomes + s) with the branch lengths[s] above each; the last record holds the two nodes that remain (an unrooted tree)."""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        n_genomes = int(n_genomes)
        m = max(n_genomes - 1, 0)
        children = np.empty(2 * m, dtype=np.int32)
        length = np.empty(2 * m, dtype=np.float32)
        self._chk(self.lib.ani_tree_nj(self.h, rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(missing_identity),
                                       children.ctypes.data if m else None, length.ctypes.data if m else None))
        return children.reshape(m, 2).astype(np.int64), length.reshape(m, 2)

    def tree_single(self, rows, n_genomes, missing_identity=0.0, return_edges=False):
        """single-linkage tree of the genomes over the pair distances min(1 - w / 100, 1 - missing_identity / 100) (ani_tree_single; the
        semantics are in ani_abi.h): `rows` as for cluster_greedy, a pair without rows at 1 - missing_identity / 100.  -> scipy linkage
        matrix, float64 (n_genomes - 1, 4), as tree_average gives it; with return_edges also `edges`, int64 (n_genomes - 1, 2): the leaf
        pair (lo < hi) that caused each merge.  The merges below the missing distance are the minimum spanning forest of the rows'
        pairs; cutting the linkage at 1 - T / 100 gives the connected components of the pairs with w >= T."""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        n_genomes = int(n_genomes)
        m = max(n_genomes - 1, 0)
        children = np.empty(2 * m, dtype=np.int32)
        height = np.empty(m, dtype=np.float32)
        edges = np.empty(2 * m, dtype=np.int32)
        self._chk(self.lib.ani_tree_single(self.h, rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(missing_identity),
                                           children.ctypes.data if m else None, height.ctypes.data if m else None,
                                           edges.ctypes.data if m and return_edges else None))
        z = self._linkage(children, height, n_genomes)
        return (z, edges.reshape(m, 2).astype(np.int64)) if return_edges else z

    def tree_support_bootstrap(self, method, rows, n_genomes, rep_identity, children, missing_identity=0.0):
        """-> uint32[n_genomes - 1]: the bootstrap support of the records of `children`, the tree of `method` ("average", "nj" or "single")
        over `rows`: per replicate r the method's tree over the rows with identity rep_identity[i, r] (float32 (len(rows), B), from
        Sketch.boot_take and boot_identity, a row without a replicate record keeping its own identity in every column), then
        tree_support, unrooted for nj (ani_tree_support_bootstrap)"""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        n_genomes = int(n_genomes)
        m = max(n_genomes - 1, 0)
        rep_identity = np.ascontiguousarray(rep_identity, dtype=np.float32)
        if rep_identity.ndim != 2 or rep_identity.shape[0] != len(rows):
            raise ValueError("rep_identity must be (len(rows), replicates)")
        children = np.ascontiguousarray(np.asarray(children).reshape(-1), dtype=np.int32)
        if len(children) != 2 * m:
            raise ValueError("children must hold n_genomes - 1 records")
        support = np.zeros(m, dtype=np.uint32)
        self._chk(self.lib.ani_tree_support_bootstrap(self.h, TREE_METHODS[method] if isinstance(method, str) else int(method),
                                                      rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(missing_identity),
                                                      rep_identity.ctypes.data if rep_identity.size else None, rep_identity.shape[1],
                                                      children.ctypes.data if m else None, support.ctypes.data if m else None))
        return support

    @staticmethod
    def _linkage(children, height, n_genomes):
        """children and height of a single-linkage call -> the scipy linkage matrix (the fourth column counts the leaves)"""
        m = max(n_genomes - 1, 0)
        z = np.empty((m, 4), dtype=np.float64)
        z[:, 0:2] = children.reshape(m, 2)
        z[:, 2] = height
        count = np.ones(n_genomes + m, dtype=np.int64)
        for s, (x, y) in enumerate(children.reshape(m, 2).tolist()):
            count[n_genomes + s] = count[x] + count[y]
        z[:, 3] = count[n_genomes:]
        return z

    def tree_single_sketch(self, rows, n_genomes, sig, length, kmer_size, min_shared=1, missing_identity=0.0, return_edges=False, return_source=False):
        """tree_single over `rows` plus, for every pair without rows, the sketch estimate signature_pairs(sig, length, kmer_size,
        min_shared) gives it if that is above 0 (ani_tree_single_sketch; the semantics are in ani_abi.h).  The sketch pairs are streamed
        through the device a strip at a time, so nothing of size n_genomes ** 2 exists anywhere and there is no 65 536 ceiling.
        -> the scipy linkage matrix as tree_single builds it; with return_edges also `edges`, int64 (n_genomes - 1, 2); with
        return_source also `source`, uint8 (n_genomes - 1,): 0 a pair with rows, 1 a sketch pair, 2 a join to leaf 0."""
        rows = np.ascontiguousarray(rows, dtype=CGI_DT)
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n_genomes = int(n_genomes)
        if sig.ndim != 2 or length.shape != (sig.shape[0],) or sig.shape[0] != max(n_genomes, 0):
            raise ValueError("sig must be (n_genomes, size) and length (n_genomes,)")
        m = max(n_genomes - 1, 0)
        children = np.empty(2 * m, dtype=np.int32)
        height = np.empty(m, dtype=np.float32)
        edges = np.empty(2 * m, dtype=np.int32)
        source = np.empty(m, dtype=np.uint8)
        self._chk(self.lib.ani_tree_single_sketch(self.h, rows.ctypes.data if len(rows) else None, len(rows), n_genomes, float(missing_identity),
                                                  sig.ctypes.data if sig.size else None, length.ctypes.data if len(length) else None, sig.shape[1],
                                                  int(kmer_size), int(min_shared), children.ctypes.data if m else None, height.ctypes.data if m else None,
                                                  edges.ctypes.data if m and return_edges else None, source.ctypes.data if m and return_source else None))
        out = (self._linkage(children, height, n_genomes),)
        if return_edges:
            out += (edges.reshape(m, 2).astype(np.int64),)
        if return_source:
            out += (source,)
        return out if len(out) > 1 else out[0]

    def tree_single_sketch_strips(self):
        """edges each strip of the last tree_single_sketch call of this engine added to its fold (ani_tree_single_sketch_strips)"""
        n = int(self.lib.ani_tree_single_sketch_strips(self.h, None, 0))
        out = np.zeros(n, dtype=np.uint64)
        if n:
            self.lib.ani_tree_single_sketch_strips(self.h, out.ctypes.data, n)
        return out

    def tree_single_rounds(self):
        """spanning-forest rounds the last tree_single call of this engine took on the device (ani_tree_single_rounds)"""
        return int(self.lib.ani_tree_single_rounds(self.h))

    def signature_pairs(self, sig, length, kmer_size, min_shared=1):
        """all pairs a < b of the signatures `sig` (uint32 (n, size), rows ascending) of lengths `length` with at least min_shared
        shared values among the first `size` of their union (ani_signature_pairs; the semantics are in ani_abi.h) -> SIGPAIR_DT
        array ordered by (a, b): shared, size and the Mash-style identity estimate at k-mer size kmer_size."""
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        if sig.ndim != 2 or length.shape != (sig.shape[0],):
            raise ValueError("sig must be (n, size) and length (n,)")
        n, size = sig.shape
        p, m = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.ani_signature_pairs(self.h, sig.ctypes.data if n else None, length.ctypes.data if n else None, n, size, int(kmer_size),
                                               int(min_shared), C.byref(p), C.byref(m)))
        return self._take(p, m.value, SIGPAIR_DT)

    def signature_neighbors(self, sig, length, kmer_size, k, min_shared=1, min_identity=0.0, rows=None):
        """for every genome of `rows` = (begin, end) (None: all of them) its k nearest neighbours among all genomes under the estimate
        of signature_pairs(sig, length, kmer_size, min_shared), identity >= min_identity, nearest first and ties by ascending id
        (ani_signature_neighbors; the semantics are in ani_abi.h).  Streamed through the device a strip of rows at a time: no 65 536
        ceiling.  -> (neighbors, count): NEIGHBOR_DT (end - begin, k), the unused slots (-1, 0, 0, 0.0), and int32 (end - begin,)."""
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        if sig.ndim != 2 or length.shape != (sig.shape[0],):
            raise ValueError("sig must be (n, size) and length (n,)")
        n, size = sig.shape
        begin, end = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        m, k = max(end - begin, 0), int(k)
        out = np.zeros((m, max(k, 0)), dtype=NEIGHBOR_DT)
        count = np.zeros(m, dtype=np.int32)
        self._chk(self.lib.ani_signature_neighbors(self.h, sig.ctypes.data if n else None, length.ctypes.data if n else None, n, size, int(kmer_size),
                                                   int(min_shared), float(min_identity), k, begin, end, out.ctypes.data if out.size else None,
                                                   count.ctypes.data if m else None))
        return out, count

    def signature_neighbors_strips(self):
        """strips the last signature_neighbors call of this engine took (ani_signature_neighbors_strips)"""
        return int(self.lib.ani_signature_neighbors_strips(self.h))

    GRAPH_ESTIMATES = {"mash": 0, "contain": 1}

    def signature_graph(self, sig, length, kmer_size, min_identity=0.0, min_shared=1, estimate="mash", rows=None):
        """the pairs a < b with a in `rows` = (begin, end) (None: all genomes) and b among all genomes that share at least min_shared
        values and whose identity is at least min_identity (ani_signature_graph; the semantics are in ani_abi.h).  estimate "mash" (0):
        the estimate of signature_pairs, so that at min_identity 0 over all rows the result is that of signature_pairs; "contain" (1):
        the symmetric containment estimate of signature_screen_contain in mode "max", the size field holding the denominator.  The
        threshold is applied on the device, a strip of rows at a time: no 65 536 ceiling.  -> SIGPAIR_DT array ordered by (a, b)."""
        if isinstance(estimate, str):
            if estimate not in self.GRAPH_ESTIMATES:
                raise ValueError("estimate %r: one of %s, or 0 .. 1" % (estimate, ", ".join(sorted(self.GRAPH_ESTIMATES))))
            estimate = self.GRAPH_ESTIMATES[estimate]
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        if sig.ndim != 2 or length.shape != (sig.shape[0],):
            raise ValueError("sig must be (n, size) and length (n,)")
        n, size = sig.shape
        begin, end = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        p, m = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.ani_signature_graph(self.h, sig.ctypes.data if n else None, length.ctypes.data if n else None, n, size, int(kmer_size),
                                               int(min_shared), float(min_identity), int(estimate), begin, end, C.byref(p), C.byref(m)))
        return self._take(p, m.value, SIGPAIR_DT)

    def signature_graph_strips(self):
        """strips the last signature_graph call of this engine took (ani_signature_graph_strips)"""
        return int(self.lib.ani_signature_graph_strips(self.h))

    def signature_screen(self, ref_sig, ref_length, qry_sig, qry_length, kmer_size, k, min_shared=1, min_identity=0.0):
        """for every query signature its k nearest references under the estimate of signature_pairs, identity >= min_identity, nearest
        first and ties by ascending reference id (ani_signature_screen; the semantics are in ani_abi.h).  Only pairs of a query and a
        reference are compared; the queries stream through the device a strip at a time, and neither side has a 65 536 ceiling.
        -> (neighbors, count): NEIGHBOR_DT (nQry, k) of reference ids, the unused slots (-1, 0, 0, 0.0), and int32 (nQry,)."""
        return self._screen(ref_sig, ref_length, qry_sig, qry_length, kmer_size, k, min_shared, min_identity, None)

    CONTAIN_MODES = {"query": 0, "reference": 1, "max": 2}

    def signature_screen_contain(self, ref_sig, ref_length, qry_sig, qry_length, kmer_size, k, mode="query", min_shared=1, min_identity=0.0):
        """signature_screen under the containment estimate (ani_signature_screen_contain; the semantics are in ani_abi.h): shared values
        over the whole of both signatures, divided by the part of one signature that lies where the other is complete.  mode "query"
        (0): how much of the query is in the reference, for partial genomes, plasmids and contigs; "reference" (1): how much of the
        reference is in the query, for references inside a larger assembly; "max" (2): the larger of the two, symmetric.
        -> (neighbors, count) as signature_screen; the size field of a record is the denominator."""
        return self._screen(ref_sig, ref_length, qry_sig, qry_length, kmer_size, k, min_shared, min_identity, self._contain_mode(mode))

    def _contain_mode(self, mode):
        """a containment mode by name or number -> its number"""
        if isinstance(mode, str):
            if mode not in self.CONTAIN_MODES:
                raise ValueError("mode %r: one of %s, or 0 .. 2" % (mode, ", ".join(sorted(self.CONTAIN_MODES))))
            mode = self.CONTAIN_MODES[mode]
        return int(mode)

    def _screen(self, ref_sig, ref_length, qry_sig, qry_length, kmer_size, k, min_shared, min_identity, mode):
        """the two screen calls: mode None is ani_signature_screen, 0 .. 2 ani_signature_screen_contain"""
        ref_sig, qry_sig = (np.ascontiguousarray(x, dtype=np.uint32) for x in (ref_sig, qry_sig))
        ref_length, qry_length = (np.ascontiguousarray(x, dtype=np.int32) for x in (ref_length, qry_length))
        if ref_sig.ndim != 2 or ref_length.shape != (ref_sig.shape[0],) or qry_sig.ndim != 2 or qry_length.shape != (qry_sig.shape[0],):
            raise ValueError("ref_sig and qry_sig must be (n, size) and the lengths (n,)")
        if ref_sig.shape[1] != qry_sig.shape[1]:
            raise ValueError("the references have signatures of size %d, the queries of size %d" % (ref_sig.shape[1], qry_sig.shape[1]))
        (nr, size), nq, k = ref_sig.shape, qry_sig.shape[0], int(k)
        out = np.zeros((nq, max(k, 0)), dtype=NEIGHBOR_DT)
        count = np.zeros(nq, dtype=np.int32)
        head = (self.h, ref_sig.ctypes.data if nr else None, ref_length.ctypes.data if nr else None, nr, qry_sig.ctypes.data if nq else None,
                qry_length.ctypes.data if nq else None, nq, size, int(kmer_size), int(min_shared), float(min_identity), k)
        tail = (out.ctypes.data if out.size else None, count.ctypes.data if nq else None)
        if mode is None:
            self._chk(self.lib.ani_signature_screen(*head, *tail))
        else:
            self._chk(self.lib.ani_signature_screen_contain(*head, mode, *tail))
        return out, count

    def signature_screen_strips(self):
        """strips the last signature_screen or signature_screen_contain call of this engine took (ani_signature_screen_strips)"""
        return int(self.lib.ani_signature_screen_strips(self.h))

    def signature_screen_tile(self):
        """(queries, references) of the merge tile of the last strip of this engine's last signature_screen or signature_screen_contain
        call (ani_signature_screen_tile)"""
        tq, tr = C.c_int32(0), C.c_int32(0)
        self.lib.ani_signature_screen_tile(self.h, C.byref(tq), C.byref(tr))
        return tq.value, tr.value

    def signature_cluster(self, sig, length, kmer_size, min_identity, min_shared=1):
        """greedy representative clustering of the genomes under the estimate of signature_pairs(sig, length, kmer_size, min_shared):
        genomes in id order, a genome is a representative iff no earlier representative is at identity >= min_identity, every other
        genome a member of its nearest representative, ties by ascending id (ani_signature_cluster; the semantics are in ani_abi.h).
        What cluster_greedy gives over the rows of signature_pairs, without the pairs: every genome is compared with the
        representatives only, and there is no 65 536 ceiling.  -> (representative, link): int32 (n,), and NEIGHBOR_DT (n,) with the
        representative, shared, size and identity of a member's pair, (-1, 0, 0, 0.0) for a representative."""
        return self._cluster(sig, length, kmer_size, min_identity, min_shared, None)

    def signature_cluster_contain(self, sig, length, kmer_size, min_identity, mode="max", min_shared=1):
        """signature_cluster under the containment estimate of signature_screen_contain (ani_signature_cluster_contain; the semantics
        are in ani_abi.h): a pair is judged by the share of the smaller genome, so that partial genomes, such as metagenome bins of
        unequal completeness, join the genome they are parts of.  mode must be "max" (2): the greedy rule needs a symmetric
        estimate, and the library refuses the other two.  -> (representative, link) as signature_cluster; the size field of a link is
        the denominator.  What cluster_greedy gives over the rows of signature_graph(estimate="contain", min_identity=0)."""
        return self._cluster(sig, length, kmer_size, min_identity, min_shared, self._contain_mode(mode))

    def _cluster(self, sig, length, kmer_size, min_identity, min_shared, mode):
        """the two cluster calls: mode None is ani_signature_cluster, otherwise ani_signature_cluster_contain"""
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        if sig.ndim != 2 or length.shape != (sig.shape[0],):
            raise ValueError("sig must be (n, size) and length (n,)")
        n, size = sig.shape
        representative = np.zeros(n, dtype=np.int32)
        link = np.zeros(n, dtype=NEIGHBOR_DT)
        head = (self.h, sig.ctypes.data if n else None, length.ctypes.data if n else None, n, size, int(kmer_size), int(min_shared), float(min_identity))
        tail = (representative.ctypes.data if n else None, link.ctypes.data if n else None)
        if mode is None:
            self._chk(self.lib.ani_signature_cluster(*head, *tail))
        else:
            self._chk(self.lib.ani_signature_cluster_contain(*head, mode, *tail))
        return representative, link

    def signature_cluster_stats(self):
        """(strips, representatives, cells walked, resolve steps) of the last signature_cluster or signature_cluster_contain call of
        this engine (ani_signature_cluster_stats); a strip's own block counts rows (rows - 1) / 2 cells where it is made from its
        upper triangle"""
        out = (C.c_uint64 * 4)()
        self._chk(self.lib.ani_signature_cluster_stats(self.h, out))
        return tuple(int(x) for x in out)


class FragmentSet:
    """Fragment sketches of a batch of query genomes kept on the device (ani_fragset)."""

    def __init__(self, engine, handle, keepalive=None):
        self.e = engine
        self.h = handle
        self._keepalive = keepalive          # the buffer a view (unpack) points into

    def info(self):
        g, f, h = C.c_int32(), C.c_int64(), C.c_uint64()
        self.e._chk(self.e.lib.ani_fragset_info(self.h, C.byref(g), C.byref(f), C.byref(h)))
        return dict(genomes=g.value, fragments=f.value, hashes=h.value)

    def packed_bytes(self):
        n = C.c_size_t()
        self.e._chk(self.e.lib.ani_fragset_pack_bytes(self.h, C.byref(n)))
        return n.value

    def pack_into(self, dev_ptr, cap):
        """the set as one device buffer (header + tables + hash pool) at dev_ptr; returns the bytes used"""
        n = C.c_size_t()
        self.e._chk(self.e.lib.ani_fragset_pack(self.e.h, self.h, dev_ptr, cap, C.byref(n)))
        return n.value

    @staticmethod
    def unpack(engine, dev_ptr, nbytes, keepalive=None):
        """view of a packed set at dev_ptr (the arrays stay in that buffer: pass its owner as keepalive)"""
        h = C.c_void_p()
        engine._chk(engine.lib.ani_fragset_unpack(engine.h, dev_ptr, nbytes, C.byref(h)))
        return FragmentSet(engine, h, keepalive)

    @staticmethod
    def unpack_merged(engine, dev_ptr, slot_bytes, slot_query_base, keepalive=None):
        """ONE set over the packed sets at dev_ptr + i * slot_bytes (an all-gather's output); slot_query_base[i] = query id of slot i's
        first genome, or -1 to leave the slot out.  Map it with first_query_id = 0."""
        q = np.ascontiguousarray(slot_query_base, dtype=np.int32)
        h = C.c_void_p()
        engine._chk(engine.lib.ani_fragset_unpack_merged(engine.h, dev_ptr, slot_bytes, len(q), q.ctypes.data, C.byref(h)))
        return FragmentSet(engine, h, keepalive)

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.ani_fragset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SketchWriter:
    """one sketch file from several sketches added one after the other (ani_sketch_writer_*): a reference set whose records exceed the
    device memory is written block by block"""
    def __init__(self, engine, path):
        self.e = engine
        h = C.c_void_p()
        engine._chk(engine.lib.ani_sketch_writer_open(str(path).encode(), C.byref(h)))
        self.h = h

    def add(self, sketch, names=None):
        arr = None
        if names is not None:
            arr = (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else n for n in names])
        self.e._chk(self.e.lib.ani_sketch_writer_add(self.h, sketch.h, arr))

    def close(self):
        if self.h:
            h, self.h = self.h, None
            self.e._chk(self.e.lib.ani_sketch_writer_close(h))

    def abort(self):
        """give the file up (it is removed)"""
        if self.h:
            h, self.h = self.h, None
            self.e.lib.ani_sketch_writer_abort(h)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False

    def __del__(self):
        try:
            self.abort()             # a writer dropped without close(): no half-written file stays behind
        except Exception:
            pass


class Sketch:
    def __init__(self, engine, params, genomes=None, records=None, record_parts=None, file=None, genome_range=(0, -1), adopt=False):
        """Either `genomes` (≙ Sketch::Sketch over the reference files), or for the multi-GPU staging path
        records=(dev_ptr, n, contig_len[int32], genome_contig_start[int32]) or
        record_parts=(dev_ptrs, counts, part_genome_start[nParts+1], contig_len, genome_contig_start); adopt=True hands the
        record buffers of record_parts over to the library (ani_sketch_adopt_record_parts: no copy for a streamed set)."""
        self.e = engine
        self.params = params
        h = C.c_void_p()
        if file is not None:
            engine._chk(engine.lib.ani_sketch_load(engine.h, str(file).encode(), genome_range[0], genome_range[1], C.byref(h)))
        elif record_parts is not None:
            ptrs, counts, pgs, clen, gcs = record_parts
            ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
            counts = np.ascontiguousarray(counts, dtype=np.uint64)
            pgs = np.ascontiguousarray(pgs, dtype=np.int32)
            clen = np.ascontiguousarray(clen, dtype=np.int32)
            gcs = np.ascontiguousarray(gcs, dtype=np.int32)
            fn = engine.lib.ani_sketch_adopt_record_parts if adopt else engine.lib.ani_sketch_from_record_parts
            engine._chk(fn(engine.h, C.byref(params), len(ptrs), ptrs.ctypes.data, counts.ctypes.data,
                        pgs.ctypes.data, clen.ctypes.data, len(clen), gcs.ctypes.data, len(gcs) - 1, C.byref(h)))
        elif records is not None:
            ptr, n, clen, gcs = records
            clen = np.ascontiguousarray(clen, dtype=np.int32)
            gcs = np.ascontiguousarray(gcs, dtype=np.int32)
            engine._chk(engine.lib.ani_sketch_from_records(engine.h, C.byref(params), ptr, n, clen.ctypes.data, len(clen),
                                                           gcs.ctypes.data, len(gcs) - 1, C.byref(h)))
        else:
            g = _as_batch(genomes)
            b = g.batch()
            engine._chk(engine.lib.ani_sketch_build(engine.h, C.byref(params), C.byref(b), C.byref(h)))
        self.h = h
        engine._sketches.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.ani_sketch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def minimizers(self):
        p, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_export(self.h, C.byref(p), C.byref(n)))
        return self.e._take(p, n.value, MINIMIZER_DT)

    def signatures(self, size=1000):
        """the `size` smallest distinct minimizer hashes of every genome (ani_sketch_signatures) -> (sig uint32 (nGenomes, size), rows
        ascending with the unused tail 0; len int32 (nGenomes,))"""
        n = self._counts()[1]
        size = int(size)
        sig = np.zeros((n, max(size, 0)), dtype=np.uint32)
        length = np.zeros(n, dtype=np.int32)
        self.e._chk(self.e.lib.ani_sketch_signatures(self.h, size, sig.ctypes.data if sig.size else None, length.ctypes.data if n else None))
        return sig, length

    def _counts(self):
        """(contigs, genomes) without the distinct-hash count that stats() computes"""
        d, f = C.c_int32(), C.c_int32()
        self.e._chk(self.e.lib.ani_sketch_stats(self.h, None, None, None, C.byref(d), C.byref(f)))
        return d.value, f.value

    def save(self, path, names=None):
        arr = None
        if names is not None:
            arr = (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else n for n in names])
        self.e._chk(self.e.lib.ani_sketch_save(self.h, str(path).encode(), arr))

    def genome_names(self):
        return [self.e.lib.ani_sketch_genome_name(self.h, g).decode() for g in range(self.stats()["genomes"])]

    def chunks(self):
        """first genome id of every index chunk of the reference set"""
        n = C.c_int32()
        self.e._chk(self.e.lib.ani_sketch_chunks(self.h, C.byref(n), None, 0))
        first = np.zeros(max(n.value, 1), dtype=np.int32)
        self.e._chk(self.e.lib.ani_sketch_chunks(self.h, C.byref(n), first.ctypes.data, n.value))
        return [int(x) for x in first[:n.value]]

    def stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        d, f = C.c_int32(), C.c_int32()
        self.e._chk(self.e.lib.ani_sketch_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(f)))
        return dict(minimizers=a.value, unique=b.value, totalLength=c.value, contigs=d.value, genomes=f.value)

    def map_query(self, genome):
        """genome = list of contigs of ONE query genome -> (mappings, totalQueryFragments)"""
        g = _as_batch([genome]) if not isinstance(genome, (HostGenomes, DeviceGenomes, UploadedGenomes)) else genome
        b = g.batch()
        p, n, tot = C.c_void_p(), C.c_size_t(), C.c_uint64()
        self.e._chk(self.e.lib.ani_map_query(self.e.h, self.h, C.byref(b), C.byref(p), C.byref(n), C.byref(tot)))
        return self.e._take(p, n.value, MAPPING_DT), tot.value

    def compute_cgi(self, mappings, total_fragments, query_id):
        m = np.ascontiguousarray(mappings, dtype=MAPPING_DT)
        p, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_compute_cgi(self.e.h, self.h, m.ctypes.data if len(m) else None, len(m), total_fragments,
                                               query_id, C.byref(p), C.byref(n)))
        return self.e._take(p, n.value, CGI_DT)

    def map_cgi_fragset(self, fragset, first_query_id=0):
        p, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_map_cgi_fragset(self.e.h, self.h, fragset.h, first_query_id, C.byref(p), C.byref(n)))
        return self.e._take(p, n.value, CGI_DT)

    def map_cgi_fragsets(self, fragsets, first_query_ids):
        """several kept sets in one call (a streamed reference set builds each index chunk once per call)"""
        hs = (C.c_void_p * len(fragsets))(*[f.h for f in fragsets])
        ids = np.ascontiguousarray(first_query_ids, dtype=np.int32)
        p, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_map_cgi_fragsets(self.e.h, self.h, len(fragsets), hs, ids.ctypes.data, C.byref(p), C.byref(n)))
        return self.e._take(p, n.value, CGI_DT)

    def set_ref_id_base(self, base):
        """this sketch is a shard / block of a larger set: CGI rows of the batch entry points report refGenomeId + base"""
        self.e._chk(self.e.lib.ani_sketch_set_ref_id_base(self.h, int(base)))

    def profile_begin(self, min_identity=0.0, min_fragments=1):
        """start (or reset) the per-bin conservation profile: every mapping call that reduces against this sketch adds its query genomes
        whose row has countSeq >= min_fragments and identity >= min_identity (ani_sketch_profile_begin)"""
        self.e._chk(self.e.lib.ani_sketch_profile_begin(self.h, float(min_identity), int(min_fragments)))

    def profile_bins(self):
        n = C.c_uint64()
        self.e._chk(self.e.lib.ani_sketch_profile_bins(self.h, C.byref(n)))
        return n.value

    def profile_read(self):
        """-> (bins BINPROFILE_DT[nBins] in set-global bin order, queries uint32[nGenomes]); does not reset"""
        bins = np.zeros(self.profile_bins(), dtype=BINPROFILE_DT)
        queries = np.zeros(self._counts()[1], dtype=np.uint32)
        self.e._chk(self.e.lib.ani_sketch_profile_read(self.h, bins.ctypes.data if len(bins) else None, queries.ctypes.data if len(queries) else None))
        return bins, queries

    def profile_end(self):
        self.e._chk(self.e.lib.ani_sketch_profile_end(self.h))

    def fragdist_begin(self, edges=(), min_identity=0.0, min_fragments=1):
        """start (or restart) the per-pair fragment identity distributions: every mapping call that reduces against this sketch appends a
        record per pair whose row has countSeq >= min_fragments and identity >= min_identity; `edges`: up to 63 ascending class edges
        in [0, 100] for the records' histograms (ani_sketch_fragdist_begin)"""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
        self.e._chk(self.e.lib.ani_sketch_fragdist_begin(self.h, float(min_identity), int(min_fragments), e.ctypes.data if len(e) else None, len(e)))
        self._fragdist_classes = len(e) + 1

    def fragdist_take(self):
        """-> (records FRAGDIST_DT[n], hist uint32[n, nEdges + 1]) appended since fragdist_begin or the last take, in row order; empties the list"""
        rp, hp, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_fragdist_take(self.h, C.byref(rp), C.byref(hp), C.byref(n)))
        k = self._fragdist_classes
        rec = self.e._take(rp, n.value, FRAGDIST_DT)
        hist = self.e._take(hp, n.value * k, np.dtype("<u4")).reshape(n.value, k)
        return rec, hist

    def fragdist_end(self):
        self.e._chk(self.e.lib.ani_sketch_fragdist_end(self.h))

    def hits_begin(self, min_identity=0.0, min_fragments=1):
        """start (or restart) the reciprocal best-hit records: every mapping call that reduces against this sketch appends one record per
        non-empty cell of every pair whose row has countSeq >= min_fragments and identity >= min_identity (ani_sketch_hits_begin)"""
        self.e._chk(self.e.lib.ani_sketch_hits_begin(self.h, float(min_identity), int(min_fragments)))

    def hits_take(self):
        """-> HIT_DT[n]: the records appended since hits_begin or the last take, pairs in row order, a pair's records in bin order; empties
        the list"""
        rp, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_hits_take(self.h, C.byref(rp), C.byref(n)))
        return self.e._take(rp, n.value, HIT_DT)

    def hits_end(self):
        self.e._chk(self.e.lib.ani_sketch_hits_end(self.h))

    def ci_begin(self, replicates=200, level=95.0, seed=1, min_identity=0.0, min_fragments=1):
        """start (or restart) the percentile bootstrap intervals of the ANI values: every mapping call that reduces against this sketch
        appends one record per pair whose row has countSeq >= min_fragments and identity >= min_identity; `replicates` in 1 .. 1024,
        `level` in percent (a multiple of 0.1 in 0.1 .. 99.9), `seed` a uint32 (ani_sketch_ci_begin)"""
        permille = float(level) * 10.0
        permille = int(round(permille)) if np.isfinite(permille) and abs(permille) < 2 ** 30 else -1
        self.e._chk(self.e.lib.ani_sketch_ci_begin(self.h, float(min_identity), int(min_fragments), int(replicates), permille, int(seed) & 0xffffffff))

    def ci_take(self):
        """-> CI_DT[n]: the records appended since ci_begin or the last take, in row order; empties the list"""
        rp, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_ci_take(self.h, C.byref(rp), C.byref(n)))
        return self.e._take(rp, n.value, CI_DT)

    def ci_end(self):
        self.e._chk(self.e.lib.ani_sketch_ci_end(self.h))

    def boot_begin(self, replicates=100, seed=1, min_identity=0.0, min_fragments=1):
        """start (or restart) the bootstrap replicate records: every mapping call that reduces against this sketch appends one record and
        `replicates` (1 .. 1024) replicate sums — the intervals' draws, kept — per pair whose row has countSeq >= min_fragments and
        identity >= min_identity; `seed` a uint32 (ani_sketch_boot_begin)"""
        self.e._chk(self.e.lib.ani_sketch_boot_begin(self.h, float(min_identity), int(min_fragments), int(replicates), int(seed) & 0xffffffff))
        self._boot_replicates = int(replicates)

    def boot_take(self):
        """-> (records BOOT_DT[n], sums uint64[n, replicates]) appended since boot_begin or the last take, in row order; empties the list"""
        rp, sp, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_boot_take(self.h, C.byref(rp), C.byref(sp), C.byref(n)))
        k = self._boot_replicates
        rec = self.e._take(rp, n.value, BOOT_DT)
        sums = self.e._take(sp, n.value * k, np.dtype("<u8")).reshape(n.value, k)
        return rec, sums

    def boot_end(self):
        self.e._chk(self.e.lib.ani_sketch_boot_end(self.h))

    def paint_begin(self):
        """start the per-fragment records: every mapping call that reduces against this sketch appends one record per query fragment
        that maps to at least one reference genome — its best reference, the runner-up and the number of genomes hit
        (ani_sketch_paint_begin); refused while the mode is on"""
        self.e._chk(self.e.lib.ani_sketch_paint_begin(self.h))

    def paint_take(self):
        """-> PAINT_DT[n]: the records appended since paint_begin or the last take, in the calls' query order, querySeqId ascending;
        empties the list"""
        rp, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_paint_take(self.h, C.byref(rp), C.byref(n)))
        return self.e._take(rp, n.value, PAINT_DT)

    def paint_end(self):
        self.e._chk(self.e.lib.ani_sketch_paint_end(self.h))

    def synteny_begin(self, min_identity=0.0, min_fragments=1):
        """start (or restart) the synteny records: every mapping call that reduces against this sketch appends, for every pair whose row
        has countSeq >= min_fragments and identity >= min_identity, one pair record (adjacency classes, blocks, reversed blocks) and one
        record per collinear block of its best hits (ani_sketch_synteny_begin)"""
        self.e._chk(self.e.lib.ani_sketch_synteny_begin(self.h, float(min_identity), int(min_fragments)))

    def synteny_take(self):
        """-> (SYNTENY_DT[nPairs], SYNBLOCK_DT[nBlocks]): the records appended since synteny_begin or the last take, pairs in row order,
        the blocks in the same pair order and per pair in bin order, pair["blocks"] of them; empties both lists"""
        pp, n, bp, m = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_sketch_synteny_take(self.h, C.byref(pp), C.byref(n), C.byref(bp), C.byref(m)))
        return self.e._take(pp, n.value, SYNTENY_DT), self.e._take(bp, m.value, SYNBLOCK_DT)

    def synteny_end(self):
        self.e._chk(self.e.lib.ani_sketch_synteny_end(self.h))

    def profile_layout(self):
        """-> (contig_bin_start int64[nContigs + 1], genome_bin_start int64[nGenomes + 1]): the first set-global bin of every contig and
        genome; contig c has contigLen[c] // (fragLen - 20) + 1 bins"""
        n_contigs, n_genomes = self._counts()
        a, b = C.c_void_p(), C.c_void_p()
        self.e._chk(self.e.lib.ani_sketch_tables(self.h, C.byref(a), C.byref(b)))
        clen = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_int32)), (n_contigs,)).astype(np.int64) if n_contigs else np.zeros(0, dtype=np.int64)
        gcs = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_int32)), (n_genomes + 1,)).astype(np.int64)
        contig_bin_start = np.concatenate([[0], np.cumsum(clen // (self.params.fragLen - 20) + 1)]).astype(np.int64)
        return contig_bin_start, contig_bin_start[gcs]

    def residency(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.e._chk(self.e.lib.ani_sketch_residency(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(streaming=bool(a.value), max_resident=b.value, resident_now=c.value)

    def map_cgi_batch(self, genomes, first_query_id=0):
        g = _as_batch(genomes)
        b = g.batch()
        p, n = C.c_void_p(), C.c_size_t()
        self.e._chk(self.e.lib.ani_map_cgi_batch(self.e.h, self.h, C.byref(b), first_query_id, C.byref(p), C.byref(n)))
        return self.e._take(p, n.value, CGI_DT)
