"""ctypes binding of libburst_host.so (C host: burst_amd/csrc/host/burst_host.h) for the tests, the bench and the
multi-GPU driver.  All logic lives in C; this module only moves pointers."""
import ctypes as C
import os
import sys

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
# BURST_AMD_LIBDIR: a directory with another build of the two libraries (tools/build_prof.sh: the phase-timer build)
LIB_PATH = os.path.join(os.environ.get("BURST_AMD_LIBDIR") or _HERE, "libburst_host.so")
MODES = {"FORAGE": 0, "BEST": 1, "ALLPATHS": 2, "CAPITALIST": 3, "ANY": 4}
REP_MERGED_LIST, REP_NO_DUPE_HUNT = 1, 2

u8p, u16p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class BhDb(C.Structure):
    _fields_ = [("rebase", C.c_int), ("xalpha", C.c_int),
                ("shear", C.c_uint32), ("totR", C.c_uint32), ("origTotR", C.c_uint32), ("numRclumps", C.c_uint32),
                ("maxLenR", C.c_uint32), ("numRefHeads", C.c_uint32),
                ("headDump", C.c_void_p), ("refHead", C.c_void_p), ("refMap", u32p), ("refStart", u32p), ("refDedupIx", u32p),
                ("tmpRIX", u32p), ("refIxSrt", u32p), ("clumpLen", u32p), ("packed", u8p), ("packedWords", C.c_uint64),
                ("hasAcx", C.c_int), ("K", C.c_int), ("acxFmt", C.c_int), ("acxZ", C.c_int),
                ("acxLens", u32p), ("acxLists", u8p), ("acxListBytes", C.c_uint64), ("badList", u32p), ("badSz", C.c_uint32),
                ("identityMap", C.c_int), ("owned", C.c_void_p * 32), ("nOwned", C.c_int), ("mapBase", C.c_void_p), ("mapLen", C.c_uint64),
                ("fragLen", u32p)]


class BhDnaStats(C.Structure):
    _fields_ = [("device", C.c_int), ("W", C.c_uint32), ("shear", C.c_uint32), ("ov", C.c_uint32), ("partitions", C.c_uint32),
                ("maxChain", C.c_uint64), ("maxSh", C.c_uint64), ("eligible", C.c_uint64), ("chunks", C.c_uint64), ("exactChunks", C.c_uint64),
                ("peakDeviceBytes", C.c_uint64), ("symbols", C.c_uint64), ("fragments", C.c_uint64),
                ("secParse", C.c_double), ("secMarks", C.c_double), ("secShear", C.c_double), ("secStages", C.c_double),
                ("secUpload", C.c_double), ("secSort", C.c_double), ("secClassify", C.c_double), ("secMark", C.c_double), ("note", C.c_char * 256)]


class BhQueries(C.Structure):
    _fields_ = [("totQ", C.c_uint64), ("numUniq", C.c_uint64), ("numEntries", C.c_uint64),
                ("dump", C.c_void_p), ("heads", C.c_void_p), ("offset", u64p), ("codes", u8p), ("codes4", u8p), ("codes2", u8p), ("len16", u16p), ("ambBefore", u32p), ("qoff", u64p),
                ("six", u32p), ("rc", u8p), ("flags", u8p), ("emac", u16p), ("len", u32p), ("ed", u16p),
                ("maxLen", C.c_uint32), ("minLen", C.c_uint32), ("maxED", C.c_uint32),
                ("nClear", C.c_uint64), ("nAmbig", C.c_uint64), ("nBad", C.c_uint64), ("pinned", C.c_int)]


class BhRun(C.Structure):
    _fields_ = [("hits", C.c_void_p), ("nHits", C.c_uint64), ("secAlign", C.c_double), ("total", capi.BhipStats), ("nBatches", C.c_uint32), ("hitsPinned", C.c_int), ("capHits", C.c_uint64),
                ("onBatch", C.c_void_p), ("onBatchCtx", C.c_void_p)]


ALIGN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, u64p, u64p, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(BhRun))
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u8p, C.c_uint64)


class BhMultiRank(C.Structure):
    _fields_ = [("rank", C.c_int), ("hh", C.c_void_p), ("r0", u64p), ("r1", u64p), ("n_ranges", C.c_uint32), ("c0", C.c_uint32), ("run", BhRun), ("secSearch", C.c_double), ("gatherPath", C.c_int),
                ("align", ALIGN_FN), ("reduce_min", REDUCE_FN), ("ctx", C.c_void_p)]


class BhRunView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("n_runs", C.c_int), ("off", C.c_uint64 * 16), ("n", C.c_uint64 * 16), ("total", C.c_uint64)]

    def runs(self):
        """the records, run by run (numpy views of the memory they lie in)"""
        out = []
        for r in range(self.n_runs):
            n = int(self.n[r])
            if n:
                buf = (C.c_uint8 * (n * capi.HIT_DTYPE.itemsize)).from_address(self.base + int(self.off[r]) * capi.HIT_DTYPE.itemsize)
                out.append(np.frombuffer(buf, dtype=capi.HIT_DTYPE))
            else:
                out.append(np.zeros(0, capi.HIT_DTYPE))
        return out


class BhTax(C.Structure):
    _fields_ = [("n", C.c_uint64), ("pair", C.c_void_p), ("blob", C.c_void_p)]


class BhTaxaTree(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_headers", C.c_uint32), ("parent", u32p), ("depth", u32p), ("header_node", u32p), ("name", C.POINTER(C.c_char_p))]


class BhTaxOpts(C.Structure):
    _fields_ = [("tax", C.POINTER(BhTax)), ("suppress", C.c_int), ("strict", C.c_int), ("taxacut", C.c_uint32), ("ncbi", C.c_int)]


class BhSessionOpts(C.Structure):
    _fields_ = [("mode", C.c_int), ("thres", C.c_float), ("do_rc", C.c_int), ("incl_ws", C.c_int), ("z", C.c_int), ("do_accel", C.c_int), ("K", C.c_int),
                ("skip_ambig", C.c_int), ("rep_flags", C.c_int), ("batch", C.c_uint64), ("shard_db", C.c_int), ("tax", C.POINTER(BhTaxOpts)),
                ("ingest_ahead", C.c_int), ("verbose", C.c_int), ("cov", C.c_void_p), ("cigar", C.c_int),
                ("mates_orientation", C.c_uint32), ("mates_ins_min", C.c_uint32), ("mates_ins_max", C.c_uint32), ("mates_report", C.c_uint32),
                ("em", C.c_void_p), ("pile", C.c_void_p)]


class BhPileRefs(C.Structure):      # the packed references as bhip_init takes them: what bh_pile_host reads the reference codes from
    _fields_ = [("packed", C.c_void_p), ("clump_len", C.c_void_p), ("n_clumps", C.c_uint32), ("tot_refs", C.c_uint32)]


class BhPathBuf(C.Structure):        # the notes of a chunk's printed lines: l = BhPathLine records (PATH_LINE_DTYPE)
    _fields_ = [("l", C.c_void_p), ("n", C.c_uint64), ("cap", C.c_uint64)]


# BhPathLine, 24 bytes: record number, refStart of the line's reference, its header number, whether its read is on this one line only
PATH_LINE_DTYPE = np.dtype({"names": ["hit", "refOff", "header", "uniq"], "formats": ["<u8", "<u4", "<u4", "<u4"], "offsets": [0, 8, 12, 16], "itemsize": 24})


class BhMatesStats(C.Structure):
    _fields_ = [("reads1", C.c_uint64), ("reads2", C.c_uint64), ("pairsNamed", C.c_uint64), ("pairsPlaced", C.c_uint64), ("lines1", C.c_uint64),
                ("lines2", C.c_uint64), ("examined", C.c_uint64), ("written", C.c_uint64), ("deviceMs", C.c_double)]


MATES_JOIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64))
E_CAPACITY = -6


COV_TAP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64)
# a solver in place of bhip_em_run (bh_em_set_solver): ctx, n_headers, n_groups, group_w, lines, n_lines, max_iters, tol, counts, info
EM_SOLVER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p)
# solvers in place of bhip_taxa_run and bhip_taxa_rollup (bh_taxa_set_solver): ctx, n_nodes, parent, n_headers, header_node, then n_groups, group_w,
# lines, n_lines, agree, group_node, own, clade, info -- or header_count, own, clade
TAXA_RUN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_void_p)
TAXA_ROLLUP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


# a solver in place of bhip_cluster_run (bh_cluster_set_solver): ctx, n_nodes, weights, edges, n_edges, centroid, edits, info
CLUSTER_SOLVER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p)


class BhSampleResult(C.Structure):
    _fields_ = [("rc", C.c_int), ("err", C.c_char * 512), ("totQ", C.c_uint64), ("numUniq", C.c_uint64), ("nHits", C.c_uint64), ("nLines", C.c_uint64),
                ("nBatches", C.c_uint32), ("secIngest", C.c_double), ("secIngestWaited", C.c_double), ("secSearch", C.c_double), ("secReport", C.c_double),
                ("total", capi.BhipStats)]


E_USAGE, E_IO, E_OOM, E_INTERNAL, E_DEVICE = -1, -2, -3, -4, -5


class HostError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        capi.lib()   # libburst_hip.so first (rpath covers it, this gives the clearer error)
        L = C.CDLL(LIB_PATH)
        L.bh_last_error.restype = C.c_char_p
        L.bh_queries_sort_device.argtypes = [C.c_int]
        L.bh_queries_sort_device.restype = None
        L.bh_queries_load.argtypes = [C.c_char_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BhQueries)]
        L.bh_queries_free.argtypes = [C.POINTER(BhQueries)]
        L.bh_queries_pin.argtypes = [C.POINTER(BhQueries)]
        L.bh_edx_read.argtypes = [C.c_char_p, C.POINTER(BhDb)]
        L.bh_acx_read.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(BhDb)]
        L.bh_db_from_fasta.argtypes = [C.c_char_p, C.c_uint32, C.c_float, C.c_int, C.c_long, C.c_int, C.POINTER(BhDb)]
        L.bh_db_from_fasta_dna.argtypes = [C.c_char_p, C.c_uint32, C.c_float, C.c_long, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(BhDb), C.POINTER(BhDnaStats)]
        L.bh_dna_marks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
        L.bh_edx_write.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_long, C.c_float]
        L.bh_acx_build.argtypes = [C.POINTER(BhDb), C.c_int, C.c_int]
        L.bh_acx_write.argtypes = [C.POINTER(BhDb), C.c_char_p]
        L.bh_db_slice.argtypes = [C.POINTER(BhDb), C.c_uint32, C.c_uint32, C.POINTER(BhDb)]
        L.bh_db_free.argtypes = [C.POINTER(BhDb)]
        L.bh_device_open.argtypes = [C.POINTER(BhDb), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_device_open_ex.argtypes = [C.POINTER(BhDb), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_device_open_shared.argtypes = [C.POINTER(BhDb), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.bh_acx_from_device.argtypes = [C.POINTER(BhDb), C.c_void_p, C.c_int, C.c_int]
        L.bh_align.argtypes = [C.c_void_p, C.POINTER(BhQueries), C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(BhRun)]
        L.bh_align_ranges.argtypes = [C.c_void_p, C.POINTER(BhQueries), u64p, u64p, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(BhRun)]
        L.bh_align_ranges_reuse.argtypes = L.bh_align_ranges.argtypes
        L.bh_search_multi.argtypes = [C.POINTER(BhMultiRank), C.c_int, C.c_int, C.c_void_p, C.POINTER(BhQueries), C.c_int, C.c_uint64, C.c_int, C.POINTER(BhRun), u64p]
        L.bh_search_multi_ex.argtypes = [C.POINTER(BhMultiRank), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BhQueries), C.c_int, C.c_uint64, C.c_int, C.POINTER(BhRun), u64p, C.POINTER(BhRunView)]
        L.bh_node_collect_view.argtypes = [C.c_void_p, C.POINTER(BhRunView), u64p]
        L.bh_report_view.argtypes = [C.c_void_p, C.POINTER(BhDb), C.POINTER(BhQueries), C.POINTER(BhRunView), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
        L.bh_node_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
        L.bh_node_close.argtypes = [C.c_void_p]
        L.bh_node_close.restype = None
        L.bh_node_attach.argtypes = [C.c_void_p, C.POINTER(BhRun)]
        L.bh_node_attach.restype = None
        L.bh_node_begin.argtypes = [C.c_void_p]
        L.bh_node_publish.argtypes = [C.c_void_p, C.POINTER(BhRun), C.c_int]
        L.bh_node_collect.argtypes = [C.c_void_p, C.POINTER(BhRun), u64p]
        L.bh_clump_shard.argtypes = [C.POINTER(BhDb), C.c_int, C.c_int, u32p, u32p]
        L.bh_clump_shard.restype = None
        L.bh_run_reserve.argtypes = [C.POINTER(BhRun), C.c_uint64]
        L.bh_run_put.argtypes = [C.POINTER(BhRun), C.c_void_p, C.c_uint64]
        L.bh_run_reserve_plain.argtypes = [C.POINTER(BhRun), C.c_uint64]
        L.bh_run_free.argtypes = [C.POINTER(BhRun)]
        L.bh_report_ex.argtypes = [C.c_void_p, C.POINTER(BhDb), C.POINTER(BhQueries), C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bh_synth_refs.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64]
        L.bh_synth_reads.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, u32p, C.c_uint32, C.c_int, C.c_double, C.c_uint64]
        L.bh_synth_refs_range.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64]
        L.bh_synth_reads_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, u32p, C.c_uint32, C.c_int, C.c_double, C.c_uint64, C.c_uint64, C.c_int]
        L.bh_edx_merge.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
        L.bh_score_lut.argtypes = [C.c_int, C.c_void_p]
        L.bh_tax_load.argtypes = [C.c_char_p, C.POINTER(BhTax)]
        L.bh_tax_free.argtypes = [C.POINTER(BhTax)]
        L.bh_tax_free.restype = None
        L.bh_session_open.argtypes = [C.POINTER(BhDb), C.POINTER(BhMultiRank), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BhSessionOpts), C.POINTER(C.c_void_p)]
        L.bh_session_prefetch.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_session_load.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(BhSampleResult)]
        L.bh_session_finish.argtypes = [C.c_void_p, C.POINTER(BhSampleResult)]
        L.bh_session_run.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(BhSampleResult)]
        L.bh_session_drop.argtypes = [C.c_void_p]
        L.bh_session_run_mates.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(BhSampleResult)]
        L.bh_session_mates.argtypes = [C.c_void_p]
        L.bh_session_mates.restype = C.c_void_p
        L.bh_mates_set_join.argtypes = [C.c_void_p, MATES_JOIN_FN, C.c_void_p]
        L.bh_mates_set_join.restype = None
        L.bh_mates_stats.argtypes = [C.c_void_p, C.POINTER(BhMatesStats)]
        L.bh_mates_stats.restype = None
        L.bh_session_sample.argtypes = [C.c_void_p]
        L.bh_session_sample.restype = C.POINTER(BhQueries)
        L.bh_session_set_node.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_session_set_node.restype = None
        L.bh_session_ended.argtypes = [C.c_void_p]
        L.bh_session_close.argtypes = [C.c_void_p]
        L.bh_paths_open.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.bh_paths_close.argtypes = [C.c_void_p]
        L.bh_paths_close.restype = None
        L.bh_paths_totals.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.bh_paths_totals.restype = None
        L.bh_cigar_text.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        L.bh_cigar_text.restype = C.c_size_t
        L.bh_report_view_paths.argtypes = [C.c_void_p, C.POINTER(BhDb), C.POINTER(BhQueries), C.POINTER(BhRunView), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64),
                                           C.c_void_p, C.c_void_p]
        L.bh_session_close.restype = None
        L.bh_cov_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.bh_cov_set_tap.argtypes = [C.c_void_p, COV_TAP_FN, C.c_void_p]
        L.bh_cov_set_tap.restype = None
        L.bh_cov_abort.argtypes = [C.c_void_p]
        L.bh_cov_abort.restype = None
        L.bh_cov_dims.argtypes = [C.c_void_p, u32p, u32p]
        L.bh_cov_dims.restype = None
        L.bh_cov_lengths.argtypes = [C.c_void_p]
        L.bh_cov_lengths.restype = u32p
        L.bh_cov_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_cov_write.argtypes = [C.c_void_p]
        L.bh_cov_close.argtypes = [C.c_void_p]
        L.bh_cov_close.restype = None
        L.bh_cov_lengths_from_extents.argtypes = [C.POINTER(BhDb), C.c_void_p, C.c_void_p]
        L.bh_cov_extents_host.argtypes = [C.POINTER(BhDb), C.c_void_p]
        L.bh_cov_extents_host.restype = None
        L.bh_cov_write_tables.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
        L.bh_em_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
        L.bh_em_open_heads.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
        L.bh_em_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_em_set_solver.restype = None
        L.bh_em_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.bh_em_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_em_abort.argtypes = [C.c_void_p]
        L.bh_em_abort.restype = None
        L.bh_em_dims.argtypes = [C.c_void_p, u32p, u32p]
        L.bh_em_dims.restype = None
        L.bh_em_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_em_write.argtypes = [C.c_void_p]
        L.bh_em_print_info.argtypes = [C.c_void_p]
        L.bh_em_print_info.restype = None
        L.bh_em_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.bh_em_last_info.restype = None
        L.bh_em_close.argtypes = [C.c_void_p]
        L.bh_em_close.restype = None
        L.bh_em_last_column.argtypes = [C.c_void_p]
        L.bh_em_last_column.restype = C.c_void_p
        L.bh_taxa_tree.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(BhTax), C.c_int, C.POINTER(BhTaxaTree)]
        L.bh_taxa_tree_free.argtypes = [C.POINTER(BhTaxaTree)]
        L.bh_taxa_tree_free.restype = None
        L.bh_taxa_check_opts.argtypes = [C.c_char_p, C.c_int, C.c_longlong]
        L.bh_taxa_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.POINTER(BhTax), C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.bh_taxa_open_heads.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(BhTax), C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.bh_taxa_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_taxa_set_solver.restype = None
        L.bh_taxa_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.bh_taxa_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_taxa_abort.argtypes = [C.c_void_p]
        L.bh_taxa_abort.restype = None
        L.bh_taxa_tree_of.argtypes = [C.c_void_p]
        L.bh_taxa_tree_of.restype = C.POINTER(BhTaxaTree)
        L.bh_taxa_dims.argtypes = [C.c_void_p, u32p, u32p]
        L.bh_taxa_dims.restype = None
        L.bh_taxa_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_taxa_write.argtypes = [C.c_void_p, u32p, u32p]
        L.bh_taxa_print_info.argtypes = [C.c_void_p]
        L.bh_taxa_print_info.restype = None
        L.bh_taxa_last_info.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_taxa_last_info.restype = None
        L.bh_taxa_close.argtypes = [C.c_void_p]
        L.bh_taxa_close.restype = None
        L.bh_taxa_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
        L.bh_taxa_rollup_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_session_set_taxa.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_em_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.bh_pile_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_pile_open_heads.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_pile_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_pile_set_solver.restype = None
        L.bh_pile_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BhPathBuf), C.c_uint64]
        L.bh_pile_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.bh_pile_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_pile_abort.argtypes = [C.c_void_p]
        L.bh_pile_abort.restype = None
        L.bh_pile_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.bh_pile_rows.restype = C.c_uint64
        L.bh_pile_write.argtypes = [C.c_void_p]
        L.bh_pile_print_info.argtypes = [C.c_void_p]
        L.bh_pile_print_info.restype = None
        L.bh_pile_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.bh_pile_last_info.restype = None
        L.bh_pile_close.argtypes = [C.c_void_p]
        L.bh_pile_close.restype = None
        L.bh_pile_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.bh_cluster_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_cluster_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_cluster_set_solver.restype = None
        L.bh_cluster_names.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32]
        L.bh_cluster_line.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint64]
        L.bh_cluster_add_b6.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_cluster_solve.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_cluster_reads.argtypes = [C.c_void_p]
        L.bh_cluster_reads.restype = C.c_uint32
        L.bh_cluster_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_cluster_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.bh_cluster_last_info.restype = None
        L.bh_cluster_write.argtypes = [C.c_void_p]
        L.bh_cluster_print_info.argtypes = [C.c_void_p]
        L.bh_cluster_print_info.restype = None
        L.bh_cluster_abort.argtypes = [C.c_void_p]
        L.bh_cluster_abort.restype = None
        L.bh_cluster_close.argtypes = [C.c_void_p]
        L.bh_cluster_close.restype = None
        L.bh_cluster_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_session_set_cluster.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_chimera_open.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.bh_chimera_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_chimera_set_solver.restype = None
        L.bh_chimera_names.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint32]
        L.bh_chimera_line.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32]
        L.bh_chimera_add_b6.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_chimera_solve.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_chimera_reads.argtypes = [C.c_void_p]
        L.bh_chimera_reads.restype = C.c_uint32
        L.bh_chimera_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_chimera_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.bh_chimera_last_info.restype = None
        L.bh_chimera_write.argtypes = [C.c_void_p]
        L.bh_chimera_print_info.argtypes = [C.c_void_p]
        L.bh_chimera_print_info.restype = None
        L.bh_chimera_abort.argtypes = [C.c_void_p]
        L.bh_chimera_abort.restype = None
        L.bh_chimera_close.argtypes = [C.c_void_p]
        L.bh_chimera_close.restype = None
        L.bh_chimera_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p]
        L.bh_session_set_chimera.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_session_set_variants.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_session_set_variants.restype = None
        L.bh_consensus_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_consensus_open_heads.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_consensus_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_consensus_set_solver.restype = None
        L.bh_consensus_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BhPathBuf), C.c_uint64]
        L.bh_consensus_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.bh_consensus_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_consensus_abort.argtypes = [C.c_void_p]
        L.bh_consensus_abort.restype = None
        L.bh_consensus_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.bh_consensus_rows.restype = C.c_uint64
        L.bh_consensus_write.argtypes = [C.c_void_p]
        L.bh_consensus_print_info.argtypes = [C.c_void_p]
        L.bh_consensus_print_info.restype = None
        L.bh_consensus_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.bh_consensus_last_info.restype = None
        L.bh_consensus_close.argtypes = [C.c_void_p]
        L.bh_consensus_close.restype = None
        L.bh_consensus_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.bh_session_set_consensus.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_conspairs_check_min.argtypes = [C.c_uint64]
        L.bh_conspairs_check_names.argtypes = [C.POINTER(C.c_char_p), C.c_uint64]
        L.bh_conspairs_open.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.bh_conspairs_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_conspairs_set_solver.restype = None
        L.bh_conspairs_attach.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_conspairs_attach.restype = None
        for name in ("bh_conspairs_abort", "bh_conspairs_print_info", "bh_conspairs_close"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.bh_conspairs_last_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.bh_conspairs_last_info.restype = None
        L.bh_conspairs_written.argtypes = [C.c_void_p]
        L.bh_consensus_pairs.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_session_consensus_pairs.argtypes = [C.c_void_p]
        L.bh_consensus_pairs_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.bh_vcf_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_vcf_open_heads.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_vcf_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_vcf_set_solver.restype = None
        L.bh_vcf_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BhPathBuf), C.c_uint64]
        L.bh_vcf_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64]
        for name in ("bh_vcf_sample_failed", "bh_vcf_abort", "bh_vcf_print_info", "bh_vcf_close"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.bh_vcf_last_info.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_vcf_last_info.restype = None
        L.bh_alleles_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.bh_session_set_vcf.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_vcfstudy_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.bh_vcfstudy_set_solver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_vcfstudy_set_solver.restype = None
        L.bh_vcfstudy_check_names.argtypes = [C.POINTER(C.c_char_p), C.c_uint64]
        L.bh_vcfstudy_add.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
        L.bh_vcfstudy_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_vcfstudy_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("bh_vcfstudy_abort", "bh_vcfstudy_print_info", "bh_vcfstudy_close"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.bh_vcfstudy_last_info.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_vcfstudy_last_info.restype = None
        L.bh_vcf_set_study.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_vcf_set_study.restype = None
        L.bh_vcf_study_sample_failed.argtypes = [C.c_void_p, C.c_char_p]
        L.bh_site_counts_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.bh_sam_open.argtypes = [C.POINTER(BhDb), C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_sam_open_heads.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.bh_sam_set_md.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bh_sam_set_md.restype = None
        L.bh_sam_begin.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BhQueries), C.c_char_p]
        L.bh_paths_set_sam.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.bh_sam_end.argtypes = [C.c_void_p]
        L.bh_sam_discard.argtypes = [C.c_void_p]
        L.bh_sam_discard.restype = None
        L.bh_sam_abort.argtypes = [C.c_void_p]
        L.bh_sam_abort.restype = None
        L.bh_sam_last_info.argtypes = [C.c_void_p, C.c_void_p]
        L.bh_sam_last_info.restype = None
        L.bh_sam_close.argtypes = [C.c_void_p]
        L.bh_sam_close.restype = None
        L.bh_md_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.bh_session_set_sam.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _taxa_tree_arrays(t):
    """names (bytes), parent, depth, header_node of a BhTaxaTree, copied"""
    n, nh = t.n_nodes, t.n_headers
    return ([t.name[v] for v in range(n)], np.ctypeslib.as_array(t.parent, (n,)).copy(), np.ctypeslib.as_array(t.depth, (n,)).copy(),
            np.ctypeslib.as_array(t.header_node, (nh,)).copy() if nh else np.zeros(0, np.uint32))


def taxa_tree(headers, taxonomy, ncbi=False):
    """bh_taxa_tree: the tree of the taxonomy map's strings for these headers (str or bytes); taxonomy: the map file of -b.  Returns (names
    as bytes, node 0 = b"Unassigned"; parent, depth uint32 [nodes]; header_node uint32 [headers]), nodes in preorder"""
    tax, tree = BhTax(), BhTaxaTree()
    _chk(lib().bh_tax_load(taxonomy.encode(), C.byref(tax)))
    try:
        hs = [h.encode() if isinstance(h, str) else bytes(h) for h in headers]
        arr = (C.c_char_p * max(len(hs), 1))(*hs)
        _chk(lib().bh_taxa_tree(len(hs), arr, C.byref(tax), int(bool(ncbi)), C.byref(tree)))
        try:
            return _taxa_tree_arrays(tree)
        finally:
            lib().bh_taxa_tree_free(C.byref(tree))
    finally:
        lib().bh_tax_free(C.byref(tax))


def taxa_host(parent, header_node, group_w, lines, agree=1000):
    """bh_taxa_host, the taxon definition in plain C (no device; candidates counted below every ancestor): (group_node uint32 [groups],
    0xFFFFFFFF = no lines; own, clade uint64 [nodes]; info uint64 [8]); lines: capi.EM_LINE_DTYPE or rows (group, ref)"""
    parent, header_node = np.ascontiguousarray(parent, dtype=np.uint32), np.ascontiguousarray(header_node, dtype=np.uint32)
    group_w = np.ascontiguousarray(group_w, dtype=np.uint32)
    lines = capi.em_lines(lines)
    nn = len(parent)
    gn, own, clade, info = np.zeros(max(len(group_w), 1), np.uint32), np.zeros(max(nn, 1), np.uint64), np.zeros(max(nn, 1), np.uint64), np.zeros(8, np.uint64)
    _chk(lib().bh_taxa_host(None, nn, parent.ctypes.data, len(header_node), header_node.ctypes.data, len(group_w), group_w.ctypes.data, lines.ctypes.data, len(lines), int(agree),
                            gn.ctypes.data, own.ctypes.data, clade.ctypes.data, info.ctypes.data))
    return gn[:len(group_w)], own[:nn], clade[:nn], info


def taxa_rollup_host(parent, header_node, header_count):
    """bh_taxa_rollup_host: counts per header summed per node and per subtree, (own, clade) uint64 [nodes]"""
    parent, header_node = np.ascontiguousarray(parent, dtype=np.uint32), np.ascontiguousarray(header_node, dtype=np.uint32)
    header_count = np.ascontiguousarray(header_count, dtype=np.uint64)
    nn = len(parent)
    own, clade = np.zeros(max(nn, 1), np.uint64), np.zeros(max(nn, 1), np.uint64)
    _chk(lib().bh_taxa_rollup_host(None, nn, parent.ctypes.data, len(header_node), header_node.ctypes.data, header_count.ctypes.data, own.ctypes.data, clade.ctypes.data))
    return own[:nn], clade[:nn]


def em_host(n_headers, group_w, lines, max_iters=1000, tol=1024):
    """bh_em_host, the abundance definition in plain C (no device): (counts uint64 [n_headers], info uint64 [8]); lines: capi.EM_LINE_DTYPE
    or rows (group, ref)"""
    group_w = np.ascontiguousarray(group_w, dtype=np.uint32)
    lines = capi.em_lines(lines)
    counts, info = np.zeros(max(int(n_headers), 1), np.uint64), np.zeros(8, np.uint64)
    _chk(lib().bh_em_host(None, int(n_headers), len(group_w), group_w.ctypes.data, lines.ctypes.data, len(lines), int(max_iters), int(tol), counts.ctypes.data, info.ctypes.data))
    return counts[:int(n_headers)], info


def cluster_host(weights, edges):
    """bh_cluster_host, the clustering definition in plain sequential C (no device): (centroid uint32 [n], edits uint32 [n], info uint64 [8]:
    0, edges kept, centroids, 0, 0, raw edges, nodes, 0).  weights: uint32 per read; edges: capi.CLUSTER_EDGE_DTYPE or rows (q, r, edits)"""
    weights = np.ascontiguousarray(weights, dtype=np.uint32)
    edges = capi.cluster_edges(edges)
    n = len(weights)
    centroid, edits, info = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(8, np.uint64)
    _chk(lib().bh_cluster_host(None, n, weights.ctypes.data, edges.ctypes.data, len(edges), centroid.ctypes.data, edits.ctypes.data, info.ctypes.data))
    return centroid[:n], edits[:n], info


class Clusterer:
    """bh_cluster.c without a run: the reads' names, lines (or a .b6 file), one solve, the two tables prefix{clusters,cluster_sizes}.txt.
    device: a capi.Device whose handle resolves the greedy order; None: bh_cluster_host (no device); solver(weights, edges) -> (centroid,
    edits): a solver of the caller's behind bh_cluster_set_solver (tests)"""

    def __init__(self, prefix, names, sizes=False, device=None, solver=None):
        self.h, self.device = C.c_void_p(), device
        _chk(lib().bh_cluster_open(prefix.encode(), int(sizes), C.byref(self.h)))
        if solver is not None:
            def _solve(ctx, n, w, e, m, centroid, edits, info):
                try:
                    wa = np.frombuffer((C.c_uint8 * (n * 4)).from_address(w), dtype=np.uint32).copy() if n else np.zeros(0, np.uint32)
                    ea = np.frombuffer((C.c_uint8 * (int(m) * 12)).from_address(e), dtype=capi.CLUSTER_EDGE_DTYPE).copy() if m else np.zeros(0, capi.CLUSTER_EDGE_DTYPE)
                    c, d = solver(wa, ea)
                    if n:
                        np.frombuffer((C.c_uint8 * (n * 4)).from_address(centroid), dtype=np.uint32)[:] = c
                        np.frombuffer((C.c_uint8 * (n * 4)).from_address(edits), dtype=np.uint32)[:] = d
                    return 0
                except Exception:      # (an exception must not cross the C frame)
                    import traceback
                    traceback.print_exc()
                    return E_DEVICE
            self._cb = CLUSTER_SOLVER_FN(_solve)
            lib().bh_cluster_set_solver(self.h, C.cast(self._cb, C.c_void_p), None)
        elif device is None:
            lib().bh_cluster_set_solver(self.h, C.cast(lib().bh_cluster_host, C.c_void_p), None)
        try:
            arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else n for n in names])
            _chk(lib().bh_cluster_names(self.h, arr, len(names)))
        except Exception:
            self.close()
            raise

    def line(self, q, ref_name, edits, count=1):
        ref_name = ref_name.encode() if isinstance(ref_name, str) else ref_name
        _chk(lib().bh_cluster_line(self.h, int(q), ref_name, len(ref_name), int(edits), int(count)))

    def add_b6(self, path):
        _chk(lib().bh_cluster_add_b6(self.h, path.encode()))

    def solve(self):
        _chk(lib().bh_cluster_solve(self.h, self.device._h if self.device is not None else None))
        return _cluster_result(self.h)

    def info(self):
        return _cluster_info(self.h)

    def write(self):
        _chk(lib().bh_cluster_write(self.h))

    def close(self):
        if self.h:
            lib().bh_cluster_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _cluster_result(h):
    n = lib().bh_cluster_reads(h)
    centroid, edits = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    _chk(lib().bh_cluster_result(h, centroid.ctypes.data, edits.ctypes.data, None))
    return centroid[:n], edits[:n]


def _cluster_info(h):
    info, lines, foreign = np.zeros(8, np.uint64), C.c_uint64(), C.c_uint64()
    lib().bh_cluster_last_info(h, info.ctypes.data, C.byref(lines), C.byref(foreign))
    d = dict(zip(capi.CLUSTER_INFO, (int(x) for x in info)))
    d["lines"], d["foreign"] = lines.value, foreign.value
    return d


def chimera_host(weights, lens, lines, ops, skew=2, min_seg=16, min_gain=3):
    """bh_chimera_host, the chimera check's definition in plain sequential C (no device): (rows capi.CHIMERA_DTYPE [n], info uint64 [8]: pairs
    kept, evaluated, chimeric, 0, 0, raw lines, nodes, 0).  weights, lens: uint32 per read; lines: capi.CHIM_LINE_DTYPE or rows (q, r, flags,
    n_ops, op_off); ops: uint32 words length << 4 | code"""
    weights = np.ascontiguousarray(weights, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    lines = capi.chim_lines(lines)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    n = len(weights)
    if len(lens) != n:
        raise ValueError("chimera_host: one length per weight")
    out, info = np.zeros(max(n, 1), capi.CHIMERA_DTYPE), np.zeros(8, np.uint64)
    _chk(lib().bh_chimera_host(None, n, weights.ctypes.data, lens.ctypes.data, lines.ctypes.data, len(lines), ops.ctypes.data, len(ops), int(skew), int(min_seg),
                               int(min_gain), out.ctypes.data, info.ctypes.data))
    return out[:n], info


class ChimeraChecker:
    """bh_chimera.c without a run: the reads' names and lengths, lines (or a .b6 file written with --cigar), one solve, the table
    prefix + chimeras.txt.  device: a capi.Device whose handle computes the profiles; None: bh_chimera_host (no device)"""

    def __init__(self, prefix, names, lens, sizes=False, skew=2, min_seg=16, min_gain=3, device=None):
        self.h, self.device = C.c_void_p(), device
        _chk(lib().bh_chimera_open(prefix.encode(), int(sizes), int(skew), int(min_seg), int(min_gain), C.byref(self.h)))
        if device is None:
            lib().bh_chimera_set_solver(self.h, C.cast(lib().bh_chimera_host, C.c_void_p), None)
        try:
            arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else n for n in names])
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            if len(lens) != len(names):
                raise ValueError("ChimeraChecker: one length per name")
            _chk(lib().bh_chimera_names(self.h, arr, lens.ctypes.data, len(names)))
        except Exception:
            self.close()
            raise

    def line(self, q, ref_name, reverse, ops):
        ref_name = ref_name.encode() if isinstance(ref_name, str) else ref_name
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        _chk(lib().bh_chimera_line(self.h, int(q), ref_name, len(ref_name), int(bool(reverse)), ops.ctypes.data, len(ops)))

    def add_b6(self, path):
        _chk(lib().bh_chimera_add_b6(self.h, path.encode()))

    def solve(self):
        _chk(lib().bh_chimera_solve(self.h, self.device._h if self.device is not None else None))
        return _chimera_result(self.h)

    def info(self):
        return _chimera_info(self.h)

    def write(self):
        _chk(lib().bh_chimera_write(self.h))

    def close(self):
        if self.h:
            lib().bh_chimera_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _chimera_result(h):
    n = lib().bh_chimera_reads(h)
    out = np.zeros(max(n, 1), capi.CHIMERA_DTYPE)
    _chk(lib().bh_chimera_result(h, out.ctypes.data, None))
    return out[:n]


def _chimera_info(h):
    info, lines, foreign = np.zeros(8, np.uint64), C.c_uint64(), C.c_uint64()
    lib().bh_chimera_last_info(h, info.ctypes.data, C.byref(lines), C.byref(foreign))
    d = dict(zip(capi.CHIMERA_INFO, (int(x) for x in info)))
    d["lines"], d["foreign"] = lines.value, foreign.value
    return d


# an MD function in place of bhip_md_tags (bh_sam_set_md): ctx, requests, ref_first, op_off, ops, n_requests, md, md_cap, md_off, nm, info
MD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p)


def md_host(lane, ref_first, ops):
    """bh_md_host, the MD definition in plain sequential C (no device): the MD string (bytes) and NM of ONE path over a lane given as an
    array of codes, lane[0] = column 1; ref_first 1-based; ops: uint32 words length << 4 | code"""
    lane = np.ascontiguousarray(lane, dtype=np.uint8)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    n, nm = C.c_uint64(0), C.c_uint32(0)
    cap = 16
    for _ in range(2):
        md = np.zeros(cap, np.uint8)
        rc = lib().bh_md_host(lane.ctypes.data, len(lane), int(ref_first), ops.ctypes.data, len(ops), md.ctypes.data, cap, C.byref(n), C.byref(nm))
        if rc != E_CAPACITY:
            break
        cap = int(n.value)
    _chk(rc)
    return md[:n.value].tobytes(), int(nm.value)


def pile_refs(packed, clump_len, tot_refs):
    """a BhPileRefs over the packed references (dbutil.pack_clumps / bhip_init's form); the arrays must outlive it (kept as attributes)"""
    r = BhPileRefs()
    r._keep = (np.ascontiguousarray(packed, dtype=np.uint8), np.ascontiguousarray(clump_len, dtype=np.uint32))
    r.packed, r.clump_len, r.n_clumps, r.tot_refs = r._keep[0].ctypes.data, r._keep[1].ctypes.data, len(r._keep[1]), int(tot_refs)
    return r


# BhConsRow, 48 bytes: a row of PREFIXconsensus.txt (header = the database's unique-header number, sample = its place in the study)
CONS_ROW_DTYPE = np.dtype([(n, "<u4") for n in ("header", "sample", "length", "covered", "called", "same", "subst", "del", "ambig", "ins_major", "record", "pad")])


def consensus_host(refs, q_codes, q_off, lines, ops, min_depth=4, seg_cap=None, letter_cap=None):
    """bh_consensus_host, the consensus definition in plain C (no device; one record per observed base): (segments capi.CONS_SEG_DTYPE,
    letters bytes, info uint64 [8]: events, candidate sites, segments, covered positions).  refs: pile_refs(...); the rest as pile_host"""
    q_codes, q_off = np.ascontiguousarray(q_codes, dtype=np.uint8), np.ascontiguousarray(q_off, dtype=np.uint64)
    lines, ops = capi.pile_lines(lines), np.ascontiguousarray(ops, dtype=np.uint32)
    seg_cap = max(len(lines), 16) if seg_cap is None else int(seg_cap)
    letter_cap = 1 << 16 if letter_cap is None else int(letter_cap)
    ns, nl, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)
    for _ in range(2):
        segs, letters = np.zeros(max(seg_cap, 1), capi.CONS_SEG_DTYPE), np.zeros(max(letter_cap, 1), np.uint8)
        rc = lib().bh_consensus_host(C.byref(refs), q_codes.ctypes.data, q_off.ctypes.data, len(q_off) - 1, lines.ctypes.data, len(lines), ops.ctypes.data, len(ops),
                                     int(min_depth), segs.ctypes.data, seg_cap, C.byref(ns), letters.ctypes.data, letter_cap, C.byref(nl), info.ctypes.data)
        if rc != E_CAPACITY or (ns.value <= seg_cap and nl.value <= letter_cap):
            break
        seg_cap, letter_cap = max(seg_cap, ns.value), max(letter_cap, nl.value)
    if rc == E_CAPACITY:
        raise HostError("bh_consensus_host: %d segments and %d letters, room for %d and %d" % (ns.value, nl.value, seg_cap, letter_cap))
    _chk(rc)
    return segs[:ns.value], letters[:nl.value].tobytes(), info


VCF_INFO = ("lines", "events", "distinct", "alleles", "snv", "del", "ins", "skipped_end", "skipped_adjacent", "skipped_long", "device_us", "peak_bytes")


CONS_PAIRS_INFO = ("samples", "failed", "records", "headers", "union_positions", "examined", "pairs", "host_bytes")


def consensus_pairs_host(n_samples, segs, letters, min_compared=1, pair_cap=None):
    """bh_consensus_pairs_host, bhip_consensus_pairs' definition in plain sequential C (no device; a dense row per (sample, header) and a
    double loop over the samples): (pairs capi.PAIR_DTYPE, info uint64 [8]).  Arguments as capi.Device.consensus_pairs takes them"""
    segs, letters = capi.pair_arrays(segs, letters)
    pair_cap = 1024 if pair_cap is None else int(pair_cap)
    for attempt in range(2):
        pairs, n, info = np.zeros(max(pair_cap, 1), capi.PAIR_DTYPE), C.c_uint64(0), np.zeros(8, np.uint64)
        rc = lib().bh_consensus_pairs_host(None, int(n_samples), segs.ctypes.data, len(segs), letters.ctypes.data, len(letters), int(min_compared), pairs.ctypes.data, pair_cap,
                                           C.byref(n), info.ctypes.data)
        if rc != E_CAPACITY or attempt:
            break
        pair_cap = int(n.value)
    _chk(rc)
    return pairs[:n.value], info


VCF_STUDY_INFO = ("samples", "failed", "snv", "del", "ins", "cells", "host_bytes", "device_us")


def site_counts_host(ranges, sites, alleles, records):
    """bh_site_counts_host, bhip_site_counts' definition in plain sequential C (no device; a loop over all ranges per record): the cells
    (capi.COUNT_CELL_DTYPE, one per record).  Arguments as capi.Device.site_counts takes them"""
    ranges, sites, alleles, records = capi.count_arrays(ranges, sites, alleles, records)
    cells, info = np.zeros(max(len(records), 1), capi.COUNT_CELL_DTYPE), np.zeros(8, np.uint64)
    _chk(lib().bh_site_counts_host(None, ranges.ctypes.data, len(ranges), sites.ctypes.data, len(sites), alleles.ctypes.data, len(alleles), records.ctypes.data, len(records),
                                   cells.ctypes.data, info.ctypes.data))
    return cells[:len(records)]


def alleles_host(refs, q_codes, q_off, lines, ops, min_depth=4, min_alt=2, cap=None, code_cap=None):
    """bh_alleles_host, the indel-allele definition in plain sequential C (no device; one record per allele run): (alleles capi.ALLELE_DTYPE,
    codes uint8, info uint64 [8]: events, distinct, returned alleles, skipped end / adjacent / long runs).  refs: pile_refs(...); the rest as
    pile_host"""
    q_codes, q_off = np.ascontiguousarray(q_codes, dtype=np.uint8), np.ascontiguousarray(q_off, dtype=np.uint64)
    lines, ops = capi.pile_lines(lines), np.ascontiguousarray(ops, dtype=np.uint32)
    cap = max(len(lines), 16) if cap is None else int(cap)
    code_cap = 1 << 12 if code_cap is None else int(code_cap)
    na, nc, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)
    for _ in range(2):
        out, codes = np.zeros(max(cap, 1), capi.ALLELE_DTYPE), np.zeros(max(code_cap, 1), np.uint8)
        rc = lib().bh_alleles_host(C.byref(refs), q_codes.ctypes.data, q_off.ctypes.data, len(q_off) - 1, lines.ctypes.data, len(lines), ops.ctypes.data, len(ops),
                                   int(min_depth), int(min_alt), out.ctypes.data, cap, C.byref(na), codes.ctypes.data, code_cap, C.byref(nc), info.ctypes.data)
        if rc != E_CAPACITY or (na.value <= cap and nc.value <= code_cap):
            break
        cap, code_cap = max(cap, na.value), max(code_cap, nc.value)
    if rc == E_CAPACITY:
        raise HostError("bh_alleles_host: %d alleles and %d codes, room for %d and %d" % (na.value, nc.value, cap, code_cap))
    _chk(rc)
    return out[:na.value], codes[:nc.value], info


def pile_host(refs, q_codes, q_off, lines, ops, min_depth=4, min_alt=2, cap=None):
    """bh_pile_host, the variant-site definition in plain C (no device; one record per observed base): (sites capi.PILE_SITE_DTYPE, info
    uint64 [8]: events, candidate sites, sites).  refs: pile_refs(...); q_codes / q_off: the query entries; lines: capi.PILE_LINE_DTYPE"""
    q_codes, q_off = np.ascontiguousarray(q_codes, dtype=np.uint8), np.ascontiguousarray(q_off, dtype=np.uint64)
    lines, ops = capi.pile_lines(lines), np.ascontiguousarray(ops, dtype=np.uint32)
    cap = max(len(lines), 16) if cap is None else int(cap)
    n, info = C.c_uint64(0), np.zeros(8, np.uint64)
    for _ in range(2):
        sites = np.zeros(max(cap, 1), capi.PILE_SITE_DTYPE)
        rc = lib().bh_pile_host(C.byref(refs), q_codes.ctypes.data, q_off.ctypes.data, len(q_off) - 1, lines.ctypes.data, len(lines), ops.ctypes.data, len(ops),
                                int(min_depth), int(min_alt), sites.ctypes.data, cap, C.byref(n), info.ctypes.data)
        if rc != E_CAPACITY or n.value <= cap:
            break
        cap = n.value
    if rc == E_CAPACITY:
        raise HostError("bh_pile_host: %d sites, room for %d" % (n.value, cap))
    _chk(rc)
    return sites[:n.value], info


def _chk(rc):
    if rc != 0:
        raise HostError("libburst_host error %d: %s" % (rc, lib().bh_last_error().decode("utf-8", "replace")))


def _view(ptr, n, dtype):
    if not n or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).view(dtype)


class Db:
    def __init__(self):
        self.c = BhDb()
        self._open = False

    @classmethod
    def read(cls, edx, acx=None, K=0, z=1):
        """K = 0: the accelerator's own K (12 or 15, from its exact size)"""
        d = cls()
        _chk(lib().bh_edx_read(edx.encode(), C.byref(d.c)))
        d._open = True
        if acx:
            _chk(lib().bh_acx_read(acx.encode(), K, z, C.byref(d.c)))
        return d

    @classmethod
    def from_fasta(cls, fasta, max_len_q, thres, shear_len=500, dedupe=True, K=None, z=1, layout="QUICK", partitions=1, device=-1, latency=16):
        """layout="DNA" (or "RNA") with shear_len: the compressive build, its duplicate marks on `device` (< 0 = the host restatement);
        the build's figures are in .dna_stats"""
        d = cls()
        if layout in ("DNA", "RNA") and shear_len:
            st = BhDnaStats()
            _chk(lib().bh_db_from_fasta_dna(fasta.encode(), max_len_q, thres, shear_len, partitions, int(dedupe), latency, device, C.byref(d.c), C.byref(st)))
            d.dna_stats = st
        elif layout in ("QUICK", "DNA", "RNA"):
            _chk(lib().bh_db_from_fasta(fasta.encode(), max_len_q, thres, 1 if shear_len else 0, shear_len or 0, int(dedupe), C.byref(d.c)))
        else:
            raise ValueError("layout must be QUICK, DNA or RNA")
        d._open = True
        d.c.identityMap = 0            # a database, not a direct-FASTA run
        if K:
            _chk(lib().bh_acx_build(C.byref(d.c), K, z))
        return d

    def write(self, edx, acx=None, db_qlen=0, thres=0.97):
        _chk(lib().bh_edx_write(C.byref(self.c), edx.encode(), db_qlen, thres))
        if acx:
            _chk(lib().bh_acx_write(C.byref(self.c), acx.encode()))

    def slice(self, c0, c1):
        """view of the clumps [c0, c1) with the accelerator restricted to them (bh_db_slice); reference index of a hit
        against the slice + 16 * c0 = index in this database"""
        d = Db()
        _chk(lib().bh_db_slice(C.byref(self.c), c0, c1, C.byref(d.c)))
        d._open = True
        d._parent = self               # the view points into the parent's clump area
        return d

    def open_device(self, device=0, z=1, build_K=0):
        """build_K > 0 for a database read without its .acx: the device builds the accelerator (bhip_init with K and no tables)"""
        h = C.c_void_p()
        _chk(lib().bh_device_open_ex(C.byref(self.c), device, z, build_K, C.byref(h)))
        dev = capi.Device.__new__(capi.Device)
        dev._h = h
        dev.n_clumps = self.c.numRclumps
        dev.clump_len = _view(self.c.clumpLen, self.c.numRclumps, np.uint32)
        return dev

    def _wrap(self, h):
        dev = capi.Device.__new__(capi.Device)
        dev._h = h
        dev.n_clumps = self.c.numRclumps
        dev.clump_len = _view(self.c.clumpLen, self.c.numRclumps, np.uint32)
        return dev

    def open_devices_team(self, devices, z=1, build_K=12):
        """This (replicated) database on len(devices) handles whose accelerator the ranks build TOGETHER: one thread per rank, as
        burst_hip --gpus N does (bh_device_open_shared with bhip_team_share: every rank the lists of its share of the words, the tables
        completed device to device).  The devices may repeat (ranks sharing a device: what a one-GPU machine can test)."""
        import threading
        n = len(devices)
        team = C.c_void_p()
        capi._chk(capi.lib().bhip_team_create(n, C.byref(team)))
        hs, rcs, errs = [C.c_void_p() for _ in range(n)], [0] * n, [""] * n
        share = C.cast(capi.lib().bhip_team_share, C.c_void_p)
        def work(r):
            rcs[r] = lib().bh_device_open_shared(C.byref(self.c), devices[r], z, build_K, r, n, share, team, C.byref(hs[r]))
            if rcs[r]:
                errs[r] = lib().bh_last_error().decode()
        ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        capi.lib().bhip_team_destroy(team)
        devs = [self._wrap(h) if not rc else None for h, rc in zip(hs, rcs)]
        if any(rcs):
            for d in devs:
                if d is not None:
                    d.close()
            raise HostError(next(rc for rc in rcs if rc), "; ".join(e for e in errs if e))
        return devs

    def open_device_shared(self, device, z, build_K, part, n_parts, share, ctx=None):
        """one of n_parts handles (one process each) that build the accelerator together; `share` = a bhip_share_fn (dist_share(...),
        or capi.lib().bhip_comm_share with ctx = a BhipCommRank)"""
        h = C.c_void_p()
        _chk(lib().bh_device_open_shared(C.byref(self.c), device, z, build_K, part, n_parts, C.cast(share, C.c_void_p), ctx, C.byref(h)))
        return self._wrap(h)

    def acx_from_device(self, dev, K, z=1):
        """accelerator tables of this database from a device handle that built them (bh_acx_from_device): write() then saves the .acx"""
        _chk(lib().bh_acx_from_device(C.byref(self.c), dev._h, K, z))

    def acx_write_from_device(self, dev, K, path, z=1):
        """the .acx of this database written straight from the tables a device handle built, list area streamed (bh_acx_write_from_device)"""
        _chk(lib().bh_acx_write_from_device(C.byref(self.c), dev._h, K, z, path.encode()))

    def close(self):
        if self._open:
            lib().bh_db_free(C.byref(self.c))
            self._open = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuerySet:
    def __init__(self, fasta, thres, rc=False, accel=True, K=12, z=1, whitespace=False):
        self.c = BhQueries()
        _chk(lib().bh_queries_load(fasta.encode(), thres, int(rc), int(whitespace), int(accel), K, z, 0, C.byref(self.c)))
        c = self.c
        self.n_reads, self.n_uniq, self.n_entries = int(c.totQ), int(c.numUniq), int(c.numEntries)

    @classmethod
    def view(cls, ptr):
        """the query tables somebody else owns (a session's current sample: what its align back end is handed), not freed here"""
        q = cls.__new__(cls)
        q.c = C.cast(ptr, C.POINTER(BhQueries)).contents
        q._borrowed = True
        q.n_reads, q.n_uniq, q.n_entries = int(q.c.totQ), int(q.c.numUniq), int(q.c.numEntries)
        return q

    def batch(self, u0=0, u1=None):
        """capi.Queries view (no copy for the forward-only case) of unique queries [u0, u1) with their RC twins"""
        c = self.c
        u1 = self.n_uniq if u1 is None else min(u1, self.n_uniq)
        qoff = _view(c.qoff, self.n_entries + 1, np.uint64)
        codes = _view(c.codes, int(qoff[-1]), np.uint8)
        ent = np.arange(u0, u1, dtype=np.int64)
        if self.n_entries > self.n_uniq:
            ent = np.concatenate([ent, ent + self.n_uniq])
        q = capi.Queries.__new__(capi.Queries)
        lens = (qoff[ent + 1] - qoff[ent]).astype(np.uint64)
        q.off = np.zeros(len(ent) + 1, np.uint64)
        np.cumsum(lens, out=q.off[1:])
        if self.n_entries == self.n_uniq:
            q.codes = codes[int(qoff[u0]):int(qoff[u1])]
        else:
            q.codes = np.concatenate([codes[int(qoff[u0]):int(qoff[u1])], codes[int(qoff[self.n_uniq + u0]):int(qoff[self.n_uniq + u1])]])
        q.emac = np.ascontiguousarray(_view(c.emac, self.n_entries, np.uint16)[ent])
        q.six = (np.ascontiguousarray(_view(c.six, self.n_entries, np.uint32)[ent]) - np.uint32(u0)).astype(np.uint32)
        q.rc = np.ascontiguousarray(_view(c.rc, self.n_entries, np.uint8)[ent])
        q.flags = np.ascontiguousarray(_view(c.flags, self.n_entries, np.uint8)[ent])
        q.n = len(ent)
        q.n_shared = u1 - u0
        q.entry_index = ent
        return q

    def pin(self):
        """page-lock the arrays the batches are copied from (bh_queries_pin)"""
        _chk(lib().bh_queries_pin(C.byref(self.c)))

    def reads_in(self, u0, u1):
        off = _view(self.c.offset, self.n_uniq + 1, np.uint64)
        return int(off[min(u1, self.n_uniq)] - off[u0])

    def close(self):
        if self.c.codes and not getattr(self, "_borrowed", False):
            lib().bh_queries_free(C.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Run:
    """records and statistics of bh_align / bh_align_ranges (the C batch scheduler: double-buffered staging, asynchronous
    hand-over of the records)"""

    def __init__(self):
        self.c = BhRun()

    @property
    def hits(self):
        n = int(self.c.nHits)
        if not n:
            return np.zeros(0, capi.HIT_DTYPE)
        buf = (C.c_uint8 * (n * capi.HIT_DTYPE.itemsize)).from_address(self.c.hits)
        return np.frombuffer(buf, dtype=capi.HIT_DTYPE)

    def stats(self):
        return self.c.total.as_dict()

    def reserve(self, cap_records):
        _chk(lib().bh_run_reserve(C.byref(self.c), int(cap_records)))

    def close(self):
        lib().bh_run_free(C.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align_ranges(dev, qs, ranges, mode, batch_uniq=1 << 18, run=None):
    """bh_align_ranges: ranges = [(u0, u1), ...] of unique queries, aligned in order through the device handle of `dev`;
    run = a Run used before: its page-locked record buffer is reused (bh_align_ranges_reuse)"""
    r0 = np.ascontiguousarray([r[0] for r in ranges], np.uint64)
    r1 = np.ascontiguousarray([r[1] for r in ranges], np.uint64)
    run = run or Run()
    _chk(lib().bh_align_ranges_reuse(dev._h, C.byref(qs.c), r0.ctypes.data_as(u64p), r1.ctypes.data_as(u64p), len(ranges), MODES[mode], batch_uniq, C.byref(run.c)))
    return run


class Node:
    """the shared-memory hand-over of the records between the ranks of one node that live in different processes (bh_node.c):
    every rank's record buffer is a segment rank 0 maps; no collective"""

    def __init__(self, job, rank, world, cap_records):
        self.h = C.c_void_p()
        _chk(lib().bh_node_open(job.encode(), rank, world, int(cap_records), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().bh_node_close(self.h)
            self.h = C.c_void_p()


class RankSearch:
    """this process's rank of a node-wide job through the C host's multi-GPU search (bh_search_multi_ex: align, [database-sharded:
    per-query minimum over the ranks,] the records to rank 0 -- through the shared-memory segments of `node`, or gathered over the
    library's RCCL communicator)"""

    def __init__(self, dev, rank, world, comm, c0=0, node=None, align=None, reduce_min=None):
        """align(ranges, mode_number) -> HIT_DTYPE records (q = global entry index, sorted by (q, refIx)): a back end in place of the
        device scheduler (the CPU tests put the oracle here; dev may then be None).  reduce_min(uint8 array) -> None: the element-wise
        minimum over all ranks, in place (database-sharded ranks in different processes without a library communicator: the
        launcher's own collective)"""
        self.mr = BhMultiRank()
        self.mr.rank, self.mr.hh, self.mr.c0 = rank, (dev._h if dev is not None else None), c0
        self.world, self.comm, self.node = world, comm, node
        self.all = Run()
        self._cb = []
        if align is not None:
            def _align(ctx, q, u0, u1, n, mode, batch, run):
                try:
                    h = np.ascontiguousarray(align([(int(u0[i]), int(u1[i])) for i in range(n)], int(mode)), dtype=capi.HIT_DTYPE)
                    return int(lib().bh_run_put(run, h.ctypes.data_as(C.c_void_p), len(h)))
                except Exception as e:      # (an exception must not cross the C frame)
                    import traceback
                    traceback.print_exc()
                    return -5
            self._cb.append(ALIGN_FN(_align))
            self.mr.align = self._cb[-1]
        if reduce_min is not None:
            def _reduce(ctx, buf, n):
                try:
                    a = np.ctypeslib.as_array(buf, shape=(int(n),))
                    reduce_min(a)
                    return 0
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return -5
            self._cb.append(REDUCE_FN(_reduce))
            self.mr.reduce_min = self._cb[-1]

    def reserve(self, cap_records):
        if self.node is None:      # (with a node the rank's buffer is its segment, sized at bh_node_open)
            _chk(lib().bh_run_reserve(C.byref(self.mr.run), int(cap_records)))

    def reserve_all(self, cap_records, pinned=False):
        """rank 0: room for everybody's records (page-locked when a device copy lands in it: the RCCL gather)"""
        _chk((lib().bh_run_reserve if pinned else lib().bh_run_reserve_plain)(C.byref(self.all.c), int(cap_records)))

    def search(self, qs, ranges, mode, batch_uniq, shard_db=False):
        """ranges: this rank's [(u0, u1), ...]; returns the gathered Run on rank 0 (its own elsewhere)"""
        r0 = np.ascontiguousarray([r[0] for r in ranges] or [0], np.uint64)
        r1 = np.ascontiguousarray([r[1] for r in ranges] or [0], np.uint64)
        self.mr.r0, self.mr.r1, self.mr.n_ranges = r0.ctypes.data_as(u64p), r1.ctypes.data_as(u64p), len(ranges)
        self._keep = (r0, r1)
        self.counts = np.zeros(self.world, np.uint64)
        self.view = BhRunView()
        n_shards = int(shard_db) if shard_db is not True else self.world      # (True: every rank its own shard)
        _chk(lib().bh_search_multi_ex(C.byref(self.mr), 1, self.world, self.comm, self.node.h if self.node is not None else None, C.byref(qs.c), MODES[mode], batch_uniq,
                                      n_shards, C.byref(self.all.c), self.counts.ctypes.data_as(u64p), C.byref(self.view)))
        return self.all      # (rank 0: self.view says where the records are -- with a node they stay in the ranks' segments)

    def own_stats(self):
        return self.mr.run.total.as_dict(), int(self.mr.run.nBatches), float(self.mr.run.secAlign)

    def close(self):
        lib().bh_run_free(C.byref(self.mr.run))
        self.all.close()
        if self.node is not None:
            self.node.close()


class Session:
    """A database that stays resident while query files run through it, each to its own .b6 (bh_session.c; burst_hip --samples):

        db = host.Db.read("DB.edx", "DB.acx")
        with host.Session(db, db.open_device(0), mode="BEST", thres=0.98) as s:
            for i, (q, out) in enumerate(samples):
                if i + 1 < len(samples):
                    s.prefetch(samples[i + 1][0])      # parsed on a thread while this one is searched and reported
                res = s.run(q, out)                    # dict: rc (0 = written), err, totQ, numUniq, nHits, nLines, seconds, stats

    devs: a device handle (Db.open_device), a list of them (the ranks are threads of this process: query-sharded, or with shard_db = S
    database-sharded over slices opened by the caller, c0 = their first clumps), or None with an `align` back end.  rank / world / node:
    one rank of a job of processes (python -m burst_amd.run).  align(qs, ranges, mode_number) -> HIT_DTYPE records: a back end in place of
    the device scheduler, handed the QuerySet of the sample being searched (the CPU tests put the oracle here); reduce_min as in RankSearch.
    accel: the queries take the accelerator's route (default: the database was read with an .acx); K: word length of a device-built
    accelerator (an .acx says its own).  A sample's usage or I/O error is its own (rc < 0 in the result, no output left); any other
    error ends the session (`ended`)."""

    def __init__(self, db, devs=None, mode="CAPITALIST", thres=0.97, rc=False, whitespace=False, z=1, accel=None, K=0, batch=1 << 21, shard_db=0,
                 taxonomy=None, taxacut=10, tax_ncbi=False, tax_suppress=False, tax_strict=False, rep_flags=0, ingest_ahead=True,
                 align=None, reduce_min=None, rank=0, world=None, c0=0, node=None, comm=None, verbose=False,
                 coverage=None, coverage_lengths=None, coverage_pad=0, coverage_tap=None, cigar=False,
                 mates_orientation="fr", insert_min=0, insert_max=1000, mates_report="all", mates_join=None,
                 abundance=None, abundance_iters=1000, abundance_tol=1024, abundance_host=False,
                 variants=None, variants_min_depth=4, variants_min_alt=2, variants_reads="all", variants_host=False,
                 cluster=None, cluster_sizes=False, cluster_host=False,
                 chimeras=None, chimera_sizes=False, chimera_skew=2, chimera_min_seg=16, chimera_min_gain=3, chimera_host=False,
                 sam=False, sam_unmapped=False, sam_lengths=None, sam_md=None,
                 consensus=None, consensus_min_depth=4, consensus_min_breadth=0, consensus_reads="all", consensus_lengths=None, consensus_host=False,
                 consensus_pairs=False, consensus_pairs_min=1, consensus_pairs_host=False,
                 vcf=False, vcf_min_depth=4, vcf_min_alt=2, vcf_reads="all", vcf_lengths=None, vcf_host=False, vcf_study=None, vcf_study_host=False,
                 taxa=None, taxa_agree=1000, taxa_host=False):
        """cigar: every line of every output carries two further columns, the leftmost 1-based position of its alignment path on the original
        reference and the path's CIGAR in =XID (bh_paths.c; traced on the handle of the rank that reports; query-sharded sessions of one
        process only).
        coverage = prefix: every reported sample feeds the coverage (bh_cov.c) on rank 0's device handle; close() writes the five tables
        prefix{shared,unique,shared_binary,unique_binary,counts}.txt unless the session ended on an error; coverage() returns the integer
        statistics.  coverage_lengths: a `name<TAB>length` table (default: the database's own extents); coverage_tap(sample, lines):
        called with every sample's placements (capi.COV_LINE_DTYPE) before they go to the device, a true return keeps them from it.
        abundance = prefix: every reported sample gets a column of the abundance table (bh_em.c: a read placed on several references split
        over them by expectation-maximisation, at most abundance_iters iterations, until no count moves by more than abundance_tol units of
        2^-30 read), solved on rank 0's device handle -- or by bh_em_host with abundance_host=True (sessions without a device); close()
        writes prefix + "abundance.txt" unless the session ended on an error; abundance() returns the integer columns.  Not with mates.
        variants = prefix: every reported sample gets a block of prefix + "variants.txt" (bh_pile.c: the reference positions where the sample's
        reads differ from the reference, counted from the alignment paths of the printed lines; listed from variants_min_depth reads on the
        position and variants_min_alt that differ; variants_reads "unique" counts only reads printed on one line), counted on rank 0's device
        handle -- or by bh_pile_host with variants_host=True; variants() returns the rows so far, close() writes the table unless the
        session ended on an error.  Opens the path tracer without adding the cigar columns; same limits as cigar.  Not with mates.
        cluster = prefix: every reported sample -- meant for ONE, the reads of the database's own FASTA, mode FORAGE -- has its reads clustered
        from the lines it prints (bh_cluster.c: greedy centroid clusters; cluster_sizes: weights from `;size=N` suffixes), resolved on rank
        0's device handle -- or by bh_cluster_host with cluster_host=True -- and prefix{clusters,cluster_sizes}.txt written at once;
        clusters() returns (centroid, edits) per read of the last sample.  FORAGE only; not with shard_db, mates, coverage, abundance, variants.
        chimeras = prefix: every reported sample -- meant for ONE, the reads of the database's own FASTA, mode FORAGE -- has its reads checked
        for two-parent chimeras from the lines it prints and their alignment paths (bh_chimera.c; chimera_sizes: weights from `;size=N`
        suffixes; chimera_skew, chimera_min_seg, chimera_min_gain: S, G and D of the definition), on rank 0's device handle -- or by
        bh_chimera_host with chimera_host=True -- and prefix + chimeras.txt written at once; chimeras() returns the rows of the last sample.
        Opens the path tracer without adding the cigar columns.  Same limits as cluster, and it goes with cluster.
        sam: every output OUT gets OUT.sam beside it (bh_sam.c: @HD, @SQ per reference header, @PG, one record per printed line with NM and
        MD tags -- bhip_md_tags on rank 0's device handle, one call per traced group); sam_unmapped: behind them a FLAG 4 record per read
        without a line, in query-file order; sam_lengths: a `name<TAB>length` table for the @SQ lines (default: the database's own extents).
        sam_md: an MD_FN in place of the device's function (tests).  Opens the path tracer without adding the cigar columns; same limits as
        cigar; goes with variants and chimeras, not with mates.  sam_info() has the last sample's figures.
        consensus = prefix: every reported sample gets a block of prefix + "consensus.fa" and prefix + "consensus.txt" (bh_consensus.c: per
        reference header the letters the sample's reads show, in reference coordinates; a position is called at consensus_min_depth reads, a
        record written at consensus_min_breadth permille of the header's length; consensus_reads "unique": only reads printed on one line;
        consensus_lengths: a `name<TAB>length` table, default the database's own extents), from ONE bhip_consensus_run per sample on rank
        0's device handle -- or bh_consensus_host with consensus_host=True; consensus() returns the table's rows so far, close() writes both
        files unless the session ended on an error.  Same limits as variants; goes with them, coverage, abundance, cigar and sam.
        consensus_pairs=True (goes with consensus=prefix): the segments and letters of every written record are kept in host memory, and
        consensus_pairs() -- or close() -- compares every two samples' rows per reference (bh_conspairs.c: Compared = positions where both
        show one of A C G T -, Same = equal ones; pair rows with Compared >= consensus_pairs_min) with ONE bhip_consensus_pairs call on rank
        0's device handle -- or bh_consensus_pairs_host with consensus_pairs_host=True -- and leaves prefix + "consensus_pairs.txt",
        "consensus_identity.txt" and "consensus_compared.txt", named together with the two consensus files by close().
        vcf: every reported sample's output OUT gets OUT.vcf beside it (bh_vcf.c: VCFv4.2, one sample, no genotypes; an SNV record where a
        base other than an A/C/G/T reference base has vcf_min_alt reads, a record per deletion and per insertion of at most 15 symbols with
        vcf_min_alt reads, at positions of vcf_min_depth reads; vcf_reads "unique": only reads printed on one line; vcf_lengths: a
        `name<TAB>length` table for the contig lines, default the database's own extents), from ONE bhip_pile_run and ONE bhip_alleles_run
        per sample on rank 0's device handle -- or bh_pile_host and bh_alleles_host with vcf_host=True.  Same limits as variants; goes with
        them, the consensus, coverage, abundance, cigar and sam.  vcf_info() has the last sample's figures.
        vcf_study = prefix (goes with vcf=True): the two calls are made at thresholds (1, 1) and filtered on the host -- OUT.vcf keeps its bytes --
        and every sample's lines (as ranges) and lists are kept in host memory; vcf_study() then writes prefix + "study.vcf" (bh_vcfstudy.c:
        a record wherever one sample's OUT.vcf has one, DP:AD of every sample at every record with no threshold applied, `.` for a sample that
        failed alone) from ONE bhip_site_counts call per sample on rank 0's device handle -- or bh_site_counts_host with vcf_study_host=True --
        and returns the figures.  close() writes it if vcf_study() was not called, unless the session ended on an error.
        taxa = prefix (needs taxonomy=): every reported sample gets a column of the taxon tables (bh_taxa.c: every read goes to the deepest
        taxonomy node that holds at least taxa_agree permille, 501 .. 1000, of the references it was placed on -- 1000: their lowest common
        ancestor), reduced on rank 0's device handle -- or by bh_taxa_host with taxa_host=True; with abundance= its counts are rolled up the
        tree as well.  close() writes prefix + "taxa.txt", "taxa_L<k>.txt" and "taxa_abundance_L<k>.txt" unless the session ended on an
        error; taxa() returns names, depths and the integer columns.  Not with mates, cluster or chimeras."""
        if vcf_study is not None and not vcf:
            raise ValueError("vcf_study goes with vcf=True")
        if (consensus_pairs or int(consensus_pairs_min) != 1) and consensus is None:
            raise ValueError("consensus_pairs and consensus_pairs_min go with consensus=prefix")
        if int(consensus_pairs_min) != 1 and not consensus_pairs:      # (as the command line refuses --consensus-pairs-min without --consensus-pairs)
            raise ValueError("consensus_pairs_min goes with consensus_pairs=True")
        if consensus_pairs and not 1 <= int(consensus_pairs_min) < 1 << 31:
            raise ValueError("consensus_pairs_min: 1 .. 2^31 - 1")
        self.db, self.h, self._cb, self.node = db, C.c_void_p(), [], node
        self._mates_join = mates_join
        self.cov, self.em, self.pile, self.cluster, self.chimera = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.sam = C.c_void_p()
        self.taxa_obj = C.c_void_p()
        devs = list(devs) if isinstance(devs, (list, tuple)) else [devs]
        n_local = len(devs)
        world = world or n_local
        c0 = list(c0) if isinstance(c0, (list, tuple)) else [c0] * n_local
        self.ranks = (BhMultiRank * n_local)()
        for i, d in enumerate(devs):
            mr = self.ranks[i]
            mr.rank, mr.hh, mr.c0 = (rank if n_local == 1 else i), (d._h if d is not None else None), c0[i]
            if align is not None:
                mr.align = self._align_cb(align)
            if reduce_min is not None:
                mr.reduce_min = self._reduce_cb(reduce_min)
        if any(d is None for d in devs) and align is None:
            raise ValueError("a session needs device handles or an align back end")
        accel = bool(db.c.hasAcx) if accel is None else bool(accel)
        self.tax, self.taxo = BhTax(), BhTaxOpts()
        o = BhSessionOpts()
        o.mode, o.thres, o.do_rc, o.incl_ws, o.z, o.do_accel, o.K = MODES[mode], thres, int(rc), int(whitespace), z, int(accel), int(db.c.K) if db.c.hasAcx else K
        o.rep_flags, o.batch, o.shard_db, o.ingest_ahead, o.verbose = rep_flags, batch, int(shard_db), int(ingest_ahead), int(verbose)
        if mates_orientation not in capi.MATES_ORIENTATIONS or mates_report not in capi.MATES_REPORTS or not 0 <= int(insert_min) <= int(insert_max) < 1 << 32:
            raise ValueError("mates: orientation fr|rf|ff, report all|best, 0 <= insert_min <= insert_max")
        o.mates_orientation, o.mates_report = capi.MATES_ORIENTATIONS[mates_orientation], capi.MATES_REPORTS[mates_report]
        o.mates_ins_min, o.mates_ins_max = int(insert_min), int(insert_max)
        if cigar:
            if shard_db and int(shard_db) > 1:
                raise ValueError("cigar: the paths are traced on one handle, which must hold the whole database (no shard_db)")
            if align is not None or world != n_local:
                raise ValueError("cigar: needs the device handles of one process (no align back end, no job of processes)")
            o.cigar = 1
        if taxonomy:
            _chk(lib().bh_tax_load(taxonomy.encode(), C.byref(self.tax)))
            self.taxo.tax, self.taxo.suppress, self.taxo.strict, self.taxo.taxacut, self.taxo.ncbi = C.pointer(self.tax), int(tax_suppress), int(tax_strict), taxacut, int(tax_ncbi)
            o.tax = C.pointer(self.taxo)
        self.ended = False
        self.cov_aborted = False
        self.cons = C.c_void_p()
        self.conspairs = C.c_void_p()
        self.vcf = C.c_void_p()
        self.vcfstudy = C.c_void_p()
        if coverage is not None and (rank == 0 or len(devs) > 1):      # (in a job of processes the lines exist only where rank 0 reports)
            _chk(lib().bh_cov_open(C.byref(db.c), coverage.encode(), coverage_lengths.encode() if coverage_lengths else None, int(coverage_pad), C.byref(self.cov)))
            if coverage_tap is not None:
                def _tap(ctx, sample, lines, n):
                    try:
                        a = np.frombuffer((C.c_uint8 * (int(n) * 16)).from_address(lines), dtype=capi.COV_LINE_DTYPE).copy() if n else np.zeros(0, capi.COV_LINE_DTYPE)
                        return 1 if coverage_tap(int(sample), a) else 0
                    except Exception:      # (an exception must not cross the C frame)
                        import traceback
                        traceback.print_exc()
                        return 0
                self._cb.append(COV_TAP_FN(_tap))
                lib().bh_cov_set_tap(self.cov, self._cb[-1], None)
            o.cov = self.cov
        if abundance is not None and (rank == 0 or len(devs) > 1):
            _chk(lib().bh_em_open(C.byref(db.c), abundance.encode(), int(abundance_iters), int(abundance_tol), C.byref(self.em)))
            if abundance_host:
                lib().bh_em_set_solver(self.em, C.cast(lib().bh_em_host, C.c_void_p), None)
            o.em = self.em
        if taxa is not None and (rank == 0 or len(devs) > 1):
            if not taxonomy:
                raise ValueError("taxa: needs the taxonomy map (taxonomy=)")
            if not 501 <= int(taxa_agree) <= 1000:
                raise ValueError("taxa: taxa_agree is the permille of a read's references that must agree, 501 .. 1000")
            if cluster is not None or chimeras is not None:
                raise ValueError("taxa: per-reference tables of a self-alignment are out of scope (no cluster, no chimeras)")
            _chk(lib().bh_taxa_open(C.byref(db.c), taxa.encode(), C.byref(self.tax), int(tax_ncbi), int(taxa_agree), C.byref(self.taxa_obj)))
            if taxa_host:
                lib().bh_taxa_set_solver(self.taxa_obj, C.cast(lib().bh_taxa_host, C.c_void_p), C.cast(lib().bh_taxa_rollup_host, C.c_void_p), None)
        if variants is not None:
            if variants_reads not in ("all", "unique") or not 1 <= int(variants_min_depth) < 1 << 31 or not 1 <= int(variants_min_alt) < 1 << 31:
                raise ValueError("variants: reads all|unique, 1 <= min_depth, min_alt < 2^31")
            if shard_db and int(shard_db) > 1:
                raise ValueError("variants: the paths are traced on one handle, which must hold the whole database (no shard_db)")
            if align is not None or world != n_local:
                raise ValueError("variants: needs the device handles of one process (no align back end, no job of processes)")
            _chk(lib().bh_pile_open(C.byref(db.c), variants.encode(), int(variants_min_depth), int(variants_min_alt), int(variants_reads == "unique"), C.byref(self.pile)))
            if variants_host:
                self._pile_refs = BhPileRefs(C.cast(db.c.packed, C.c_void_p), C.cast(db.c.clumpLen, C.c_void_p), db.c.numRclumps, db.c.totR)
                lib().bh_pile_set_solver(self.pile, C.cast(lib().bh_pile_host, C.c_void_p), C.cast(C.pointer(self._pile_refs), C.c_void_p))
            o.pile = self.pile
        if cluster is not None:
            if mode != "FORAGE":
                raise ValueError("cluster: needs every relationship under the identity cutoff: mode FORAGE")
            if (shard_db and int(shard_db) > 1) or align is not None or world != n_local:
                raise ValueError("cluster: needs the whole report and the device handles of one process (no shard_db, no align back end, no job of processes)")
            if coverage is not None or abundance is not None or variants is not None:
                raise ValueError("cluster: per-reference tables of a self-alignment are out of scope (no coverage, abundance, variants)")
            _chk(lib().bh_cluster_open(cluster.encode(), int(bool(cluster_sizes)), C.byref(self.cluster)))
            if cluster_host:
                lib().bh_cluster_set_solver(self.cluster, C.cast(lib().bh_cluster_host, C.c_void_p), None)
        if chimeras is not None:
            if mode != "FORAGE":
                raise ValueError("chimeras: needs every relationship under the identity cutoff: mode FORAGE")
            if (shard_db and int(shard_db) > 1) or align is not None or world != n_local:
                raise ValueError("chimeras: needs the whole report and the device handles of one process (no shard_db, no align back end, no job of processes)")
            if coverage is not None or abundance is not None or variants is not None:
                raise ValueError("chimeras: per-reference tables of a self-alignment are out of scope (no coverage, abundance, variants)")
            _chk(lib().bh_chimera_open(chimeras.encode(), int(bool(chimera_sizes)), int(chimera_skew), int(chimera_min_seg), int(chimera_min_gain), C.byref(self.chimera)))
            if chimera_host:
                lib().bh_chimera_set_solver(self.chimera, C.cast(lib().bh_chimera_host, C.c_void_p), None)
        if consensus is not None:
            if consensus_reads not in ("all", "unique") or not 1 <= int(consensus_min_depth) < 1 << 31 or not 0 <= int(consensus_min_breadth) <= 1000:
                raise ValueError("consensus: reads all|unique, 1 <= min_depth < 2^31, 0 <= min_breadth <= 1000")
            if shard_db and int(shard_db) > 1:
                raise ValueError("consensus: the paths are traced on one handle, which must hold the whole database (no shard_db)")
            if align is not None or world != n_local:
                raise ValueError("consensus: needs the device handles of one process (no align back end, no job of processes)")
            if cluster is not None or chimeras is not None:
                raise ValueError("consensus: per-reference outputs of a self-alignment are out of scope (no cluster, no chimeras)")
            _chk(lib().bh_consensus_open(C.byref(db.c), consensus.encode(), consensus_lengths.encode() if consensus_lengths else None, int(consensus_min_depth),
                                         int(consensus_min_breadth), int(consensus_reads == "unique"), C.byref(self.cons)))
            if consensus_host:
                self._cons_refs = BhPileRefs(C.cast(db.c.packed, C.c_void_p), C.cast(db.c.clumpLen, C.c_void_p), db.c.numRclumps, db.c.totR)
                lib().bh_consensus_set_solver(self.cons, C.cast(lib().bh_consensus_host, C.c_void_p), C.cast(C.pointer(self._cons_refs), C.c_void_p))
            if consensus_pairs:
                _chk(lib().bh_conspairs_open(consensus.encode(), int(consensus_pairs_min), C.byref(self.conspairs)))
                if consensus_pairs_host:
                    lib().bh_conspairs_set_solver(self.conspairs, C.cast(lib().bh_consensus_pairs_host, C.c_void_p), None)
                lib().bh_conspairs_attach(self.conspairs, self.cons)
        if vcf_lengths and not vcf:
            raise ValueError("vcf_lengths goes with vcf=True")
        if vcf:
            if vcf_reads not in ("all", "unique") or not 1 <= int(vcf_min_depth) < 1 << 31 or not 1 <= int(vcf_min_alt) < 1 << 31:
                raise ValueError("vcf: reads all|unique, 1 <= min_depth < 2^31, 1 <= min_alt < 2^31")
            if shard_db and int(shard_db) > 1:
                raise ValueError("vcf: the paths are traced on one handle, which must hold the whole database (no shard_db)")
            if align is not None or world != n_local:
                raise ValueError("vcf: needs the device handles of one process (no align back end, no job of processes)")
            if cluster is not None or chimeras is not None:
                raise ValueError("vcf: per-reference outputs of a self-alignment are out of scope (no cluster, no chimeras)")
            _chk(lib().bh_vcf_open(C.byref(db.c), vcf_lengths.encode() if vcf_lengths else None, int(vcf_min_depth), int(vcf_min_alt), int(vcf_reads == "unique"), C.byref(self.vcf)))
            if vcf_host:
                self._vcf_refs = BhPileRefs(C.cast(db.c.packed, C.c_void_p), C.cast(db.c.clumpLen, C.c_void_p), db.c.numRclumps, db.c.totR)
                ctx = C.cast(C.pointer(self._vcf_refs), C.c_void_p)
                lib().bh_vcf_set_solver(self.vcf, C.cast(lib().bh_pile_host, C.c_void_p), ctx, C.cast(lib().bh_alleles_host, C.c_void_p), ctx)
        if vcf_study is not None:
            _chk(lib().bh_vcfstudy_open(str(vcf_study).encode(), C.byref(self.vcfstudy)))
            if vcf_study_host:
                lib().bh_vcfstudy_set_solver(self.vcfstudy, C.cast(lib().bh_site_counts_host, C.c_void_p), None)
            lib().bh_vcf_set_study(self.vcf, self.vcfstudy)
        if (sam_unmapped or sam_lengths) and not sam:
            raise ValueError("sam_unmapped and sam_lengths go with sam=True")
        if sam:
            if shard_db and int(shard_db) > 1:
                raise ValueError("sam: the paths are traced on one handle, which must hold the whole database (no shard_db)")
            if align is not None or world != n_local:
                raise ValueError("sam: needs the device handles of one process (no align back end, no job of processes)")
            _chk(lib().bh_sam_open(C.byref(db.c), sam_lengths.encode() if sam_lengths else None, int(bool(sam_unmapped)), C.byref(self.sam)))
            if sam_md is not None:
                self._cb.append(sam_md)
                lib().bh_sam_set_md(self.sam, C.cast(sam_md, C.c_void_p), None)
        try:
            _chk(lib().bh_session_open(C.byref(db.c), self.ranks, n_local, world, comm, node.h if node is not None else None, C.byref(o), C.byref(self.h)))
            if self.sam:
                _chk(lib().bh_session_set_sam(self.h, self.sam))
            if self.cons:
                _chk(lib().bh_session_set_consensus(self.h, self.cons))
            if self.vcf:
                _chk(lib().bh_session_set_vcf(self.h, self.vcf))
            if self.taxa_obj:
                _chk(lib().bh_session_set_taxa(self.h, self.taxa_obj))
            if self.cluster:
                _chk(lib().bh_session_set_cluster(self.h, self.cluster))
            if self.chimera:
                _chk(lib().bh_session_set_chimera(self.h, self.chimera))
        except Exception:      # (the objects opened above belong to a session that will never be closed: release them here)
            if self.h:
                lib().bh_session_close(self.h)
                self.h = C.c_void_p()
            for name, close in (("sam", lib().bh_sam_close), ("taxa_obj", lib().bh_taxa_close), ("vcfstudy", lib().bh_vcfstudy_close), ("vcf", lib().bh_vcf_close), ("cons", lib().bh_consensus_close), ("conspairs", lib().bh_conspairs_close), ("cluster", lib().bh_cluster_close), ("chimera", lib().bh_chimera_close)):
                if getattr(self, name):
                    close(getattr(self, name))
                    setattr(self, name, C.c_void_p())
            raise

    def _align_cb(self, align):
        def _align(ctx, q, u0, u1, n, mode, batch, run):
            try:
                h = np.ascontiguousarray(align(QuerySet.view(q), [(int(u0[i]), int(u1[i])) for i in range(n)], int(mode)), dtype=capi.HIT_DTYPE)
                return int(lib().bh_run_put(run, h.ctypes.data_as(C.c_void_p), len(h)))
            except Exception:      # (an exception must not cross the C frame)
                import traceback
                traceback.print_exc()
                return E_DEVICE
        self._cb.append(ALIGN_FN(_align))
        return self._cb[-1]

    def _reduce_cb(self, reduce_min):
        def _reduce(ctx, buf, n):
            try:
                reduce_min(np.ctypeslib.as_array(buf, shape=(int(n),)))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return E_DEVICE
        self._cb.append(REDUCE_FN(_reduce))
        return self._cb[-1]

    @staticmethod
    def _result(res):
        d = {k: getattr(res, k) for k in ("rc", "totQ", "numUniq", "nHits", "nLines", "nBatches", "secIngest", "secIngestWaited", "secSearch", "secReport")}
        d["err"] = res.err.decode("utf-8", "replace")
        d["stats"] = res.total.as_dict()
        return d

    def _done(self, rc, res):
        self.ended = bool(lib().bh_session_ended(self.h))
        return self._result(res)

    def prefetch(self, queries):
        _chk(lib().bh_session_prefetch(self.h, queries.encode()))

    def _mates_cb(self, join):
        def _join(ctx, a, na, b, nb, orientation, ins_min, ins_max, report, out_a, out_b, cap, n_out):
            try:
                la = np.frombuffer((C.c_uint8 * (int(na) * 20)).from_address(a), dtype=capi.MATE_LINE_DTYPE) if na else np.zeros(0, capi.MATE_LINE_DTYPE)
                lb = np.frombuffer((C.c_uint8 * (int(nb) * 20)).from_address(b), dtype=capi.MATE_LINE_DTYPE) if nb else np.zeros(0, capi.MATE_LINE_DTYPE)
                r = join(la, lb, int(orientation), int(ins_min), int(ins_max), int(report), int(cap))
                if isinstance(r, int):      # (the joiner asks for room)
                    n_out[0] = r
                    return E_CAPACITY
                ia, ib = (np.ascontiguousarray(x, dtype=np.uint32) for x in r)
                n_out[0] = len(ia)
                if len(ia) > cap:
                    return E_CAPACITY
                C.memmove(out_a, ia.ctypes.data, 4 * len(ia))
                C.memmove(out_b, ib.ctypes.data, 4 * len(ib))
                return 0
            except Exception:      # (an exception must not cross the C frame)
                import traceback
                traceback.print_exc()
                return E_INTERNAL
        self._cb.append(MATES_JOIN_FN(_join))
        return self._cb[-1]

    def run(self, queries, out, mates=None):
        """mates: the second mate file -- `queries` and `mates` are searched one after the other and `out` gets their concordant combinations
        (bh_session_run_mates; the session's mates_orientation, insert_min, insert_max, mates_report; needs mode ALLPATHS or FORAGE and
        rc=True).  The result then has "mates": reads1, reads2, pairsNamed, pairsPlaced, lines1, lines2, examined, written, deviceMs.
        mates_join(a, b, orientation, ins_min, ins_max, report, cap) -> (out_a, out_b), or an int = room wanted: a joiner in place of the
        device's (the CPU tests put the definition's brute force here)"""
        res = BhSampleResult()
        if mates is not None:
            m = lib().bh_session_mates(self.h)
            if m and self._mates_join is not None:
                lib().bh_mates_set_join(m, self._mates_cb(self._mates_join), None)
                self._mates_join = None
            d = self._done(lib().bh_session_run_mates(self.h, queries.encode(), mates.encode(), out.encode() if out else None, C.byref(res)), res)
            if m and not d["rc"]:
                st = BhMatesStats()
                lib().bh_mates_stats(m, C.byref(st))
                d["mates"] = {k: getattr(st, k) for k, _ in BhMatesStats._fields_}
            return d
        return self._done(lib().bh_session_run(self.h, queries.encode(), out.encode() if out else None, C.byref(res)), res)

    def load(self, queries, out):
        """first half of run(): the sample's tables are in hand (`sample`), its output is created; finish() or drop() must follow"""
        res = BhSampleResult()
        return self._done(lib().bh_session_load(self.h, queries.encode(), out.encode() if out else None, C.byref(res)), res)

    def finish(self):
        res = BhSampleResult()
        return self._done(lib().bh_session_finish(self.h, C.byref(res)), res)

    def drop(self):
        lib().bh_session_drop(self.h)

    @property
    def sample(self):
        p = lib().bh_session_sample(self.h)
        return QuerySet.view(p) if p else None

    def set_node(self, node):
        self.node = node
        lib().bh_session_set_node(self.h, node.h if node is not None else None)

    def coverage(self):
        """the integer statistics so far: (shared, unique), each uint64 [columns][headers][4] = tot, cov, sq, lines; column 0 = Dataset"""
        if not self.cov:
            raise HostError("the session has no coverage")
        nc, nh = C.c_uint32(), C.c_uint32()
        lib().bh_cov_dims(self.cov, C.byref(nc), C.byref(nh))
        sh, un = np.zeros((nc.value, nh.value, 4), np.uint64), np.zeros((nc.value, nh.value, 4), np.uint64)
        _chk(lib().bh_cov_stats(self.cov, sh.ctypes.data, un.ctypes.data))
        return sh, un

    def abundance(self):
        """the abundance columns so far: uint64 [columns][headers] in units of 2^-30 read; column 0 = Dataset, the sum of the sample columns"""
        if not self.em:
            raise HostError("the session has no abundance")
        nc, nh = C.c_uint32(), C.c_uint32()
        lib().bh_em_dims(self.em, C.byref(nc), C.byref(nh))
        cols = np.zeros((nc.value, nh.value), np.uint64)
        _chk(lib().bh_em_stats(self.em, cols.ctypes.data))
        return cols

    def taxa(self):
        """the taxon tables so far: dict of names (bytes per node, node 0 = b"Unassigned"), parent, depth, header_node and the uint64 columns
        own, clade, own_em, clade_em, each [columns][nodes] with column 0 = Dataset (the _em ones in units of 2^-30 read, zero without abundance)"""
        if not self.taxa_obj:
            raise HostError("the session has no taxa")
        nc, nn = C.c_uint32(), C.c_uint32()
        lib().bh_taxa_dims(self.taxa_obj, C.byref(nc), C.byref(nn))
        cols = np.zeros((4, nc.value, nn.value), np.uint64)
        _chk(lib().bh_taxa_stats(self.taxa_obj, cols.ctypes.data))
        names, parent, depth, hn = _taxa_tree_arrays(lib().bh_taxa_tree_of(self.taxa_obj).contents)
        return dict(names=names, parent=parent, depth=depth, header_node=hn, own=cols[0], clade=cols[1], own_em=cols[2], clade_em=cols[3])

    def taxa_info(self):
        """the last sample's figures: pairs, groups, reads, root_reads, deepest, device_us, peak_bytes"""
        info = np.zeros(8, np.uint64)
        lib().bh_taxa_last_info(self.taxa_obj, info.ctypes.data)
        return dict(zip(("pairs", "groups", "reads", "root_reads", "deepest", "device_us", "peak_bytes"), (int(x) for x in info)))

    def abundance_info(self):
        """the last solved sample's figures: iterations, pairs, classes, delta, converged, device_us, peak_bytes, reads"""
        info, reads = np.zeros(8, np.uint64), C.c_uint64()
        lib().bh_em_last_info(self.em, info.ctypes.data, C.byref(reads))
        d = dict(zip(("iterations", "pairs", "classes", "delta", "converged", "device_us", "peak_bytes"), (int(x) for x in info)))
        d["reads"] = reads.value
        return d

    def variants(self):
        """the rows of the variants table so far: (sites capi.PILE_SITE_DTYPE with header = the database's unique-header number, sample uint32
        per row), in the table's order"""
        if not self.pile:
            raise HostError("the session has no variants")
        n = lib().bh_pile_rows(self.pile, None, None, 0)
        rows, samples = np.zeros(max(n, 1), capi.PILE_SITE_DTYPE), np.zeros(max(n, 1), np.uint32)
        lib().bh_pile_rows(self.pile, rows.ctypes.data, samples.ctypes.data, n)
        return rows[:n], samples[:n]

    def variants_info(self):
        """the last counted sample's figures: events, candidates, sites, device_us, peak_bytes, lines"""
        info, lines = np.zeros(8, np.uint64), C.c_uint64()
        lib().bh_pile_last_info(self.pile, info.ctypes.data, C.byref(lines))
        d = dict(zip(capi.PILE_INFO, (int(x) for x in info)))
        d["lines"] = lines.value
        return d

    def consensus(self):
        """the rows of the consensus table so far (CONS_ROW_DTYPE: header = the database's unique-header number, sample = its place in the study,
        length, covered, called, same, subst, del, ambig, ins_major, record), in the table's order"""
        if not self.cons:
            raise HostError("the session has no consensus")
        n = lib().bh_consensus_rows(self.cons, None, 0)
        rows = np.zeros(max(n, 1), CONS_ROW_DTYPE)
        lib().bh_consensus_rows(self.cons, rows.ctypes.data, n)
        return rows[:n]

    def consensus_pairs(self):
        """when every sample has been reported: ONE bhip_consensus_pairs call over the kept rows on rank 0's device handle (or
        bh_consensus_pairs_host with consensus_pairs_host=True) and prefix + "consensus_pairs.txt", "consensus_identity.txt" and
        "consensus_compared.txt" under temporary names (once: the kept rows are released, and no further sample can be reported); close()
        gives them and the two consensus files their names together.  Returns the figures: samples (done), failed, records (that take
        part), headers (with two or more), union_positions, examined, pairs (written), host_bytes (kept), device_us"""
        if not self.conspairs:
            raise HostError("the session has no consensus pairs")
        if lib().bh_session_ended(self.h):
            raise HostError("the session ended on an error: no consensus pairs are written")
        _chk(lib().bh_session_consensus_pairs(self.h))
        return self.consensus_pairs_info()

    def consensus_pairs_info(self):
        info, us = np.zeros(8, np.uint64), C.c_uint64()
        lib().bh_conspairs_last_info(self.conspairs, info.ctypes.data, C.byref(us))
        d = dict(zip(CONS_PAIRS_INFO, (int(x) for x in info)))
        d["device_us"] = us.value
        return d

    def consensus_info(self):
        """the last called sample's figures: events, candidates, segments, covered, device_us, peak_bytes, lines, records"""
        info, lines, records = np.zeros(8, np.uint64), C.c_uint64(), C.c_uint64()
        lib().bh_consensus_last_info(self.cons, info.ctypes.data, C.byref(lines), C.byref(records))
        d = dict(zip(capi.CONS_INFO, (int(x) for x in info)))
        d["lines"], d["records"] = lines.value, records.value
        return d

    def clusters(self):
        """the last sample's clustering: (centroid uint32 [reads], edits uint32 [reads]) per read in file order -- the number of its centroid
        (its own for a centroid) and the edits of the line that joined it"""
        if not self.cluster:
            raise HostError("the session has no clustering")
        return _cluster_result(self.cluster)

    def clusters_info(self):
        """the last clustering's figures: rounds, edges_kept, centroids, device_us, device_bytes, edges, nodes, lines, foreign"""
        return _cluster_info(self.cluster)

    def chimeras(self):
        """the last sample's chimera check: a capi.CHIMERA_DTYPE row per read in file order (role 0 not evaluated, 1 N, 2 Y)"""
        if not self.chimera:
            raise HostError("the session has no chimera check")
        return _chimera_result(self.chimera)

    def chimeras_info(self):
        """the last chimera check's figures: pairs_kept, evaluated, chimeric, device_us, device_bytes, lines (given to the device), nodes,
        lines (printed), foreign"""
        return _chimera_info(self.chimera)

    def vcf_info(self):
        """the last written sample's figures: lines, events, distinct, alleles, snv, del, ins (records), skipped_end, skipped_adjacent,
        skipped_long, device_us, peak_bytes"""
        info = np.zeros(12, np.uint64)
        lib().bh_vcf_last_info(self.vcf, info.ctypes.data)
        return dict(zip(VCF_INFO, (int(x) for x in info)))

    def vcf_study(self):
        """writes prefix + "study.vcf" from the samples reported so far (once: the kept lists are released) and returns the figures: samples
        (done), failed, snv, del, ins (records), cells, host_bytes (kept), device_us"""
        if not self.vcfstudy:
            raise HostError("the session has no study VCF")
        if lib().bh_session_ended(self.h):
            raise HostError("the session ended on an error: no study VCF is written")
        _chk(lib().bh_vcfstudy_write(self.vcfstudy, self.vcf, self.ranks[0].hh))
        self._vcfstudy_written = True
        return self.vcf_study_info()

    def vcf_study_info(self):
        info = np.zeros(8, np.uint64)
        lib().bh_vcfstudy_last_info(self.vcfstudy, info.ctypes.data)
        return dict(zip(VCF_STUDY_INFO, (int(x) for x in info)))

    def sam_info(self):
        """the last written sample's figures: records, unmapped, md_bytes, device_us"""
        info = np.zeros(4, np.uint64)
        lib().bh_sam_last_info(self.sam, info.ctypes.data)
        return dict(zip(("records", "unmapped", "md_bytes", "device_us"), (int(x) for x in info)))

    def coverage_abort(self):
        """the walk ends on an error that the session itself has not seen (another rank's): close() writes no tables"""
        if self.cov:
            lib().bh_cov_abort(self.cov)
            self.cov_aborted = True

    def coverage_lengths(self):
        nh = C.c_uint32()
        lib().bh_cov_dims(self.cov, None, C.byref(nh))
        p = lib().bh_cov_lengths(self.cov)
        return _view(p, nh.value, np.uint32).copy() if p else None

    def close(self):
        if self.h:
            err = None
            if self.cov:      # (before the handles go: the coverage lives on rank 0's)
                if not lib().bh_session_ended(self.h) and not self.cov_aborted and lib().bh_cov_write(self.cov):
                    err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_cov_close(self.cov)
                self.cov = C.c_void_p()
            if self.em:
                if not lib().bh_session_ended(self.h) and not self.cov_aborted and lib().bh_em_write(self.em):
                    err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_em_close(self.em)
                self.em = C.c_void_p()
            if self.taxa_obj:
                if not lib().bh_session_ended(self.h) and not self.cov_aborted and lib().bh_taxa_write(self.taxa_obj, None, None):
                    err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_taxa_close(self.taxa_obj)
                self.taxa_obj = C.c_void_p()
            if self.pile:
                if not lib().bh_session_ended(self.h) and not self.cov_aborted and lib().bh_pile_write(self.pile):
                    err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_pile_close(self.pile)
                self.pile = C.c_void_p()
            if self.cons:
                if not lib().bh_session_ended(self.h) and not self.cov_aborted:     # (the pairs before the handles go, then all files get their names)
                    if (self.conspairs and not lib().bh_conspairs_written(self.conspairs) and lib().bh_session_consensus_pairs(self.h)) or lib().bh_consensus_write(self.cons):
                        err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_consensus_close(self.cons)
                self.cons = C.c_void_p()
                if self.conspairs:
                    lib().bh_conspairs_close(self.conspairs)
                    self.conspairs = C.c_void_p()
            if self.vcfstudy:     # (before the handles go: the counts are taken on rank 0's)
                if not getattr(self, "_vcfstudy_written", False) and not lib().bh_session_ended(self.h) and not self.cov_aborted and lib().bh_vcfstudy_write(self.vcfstudy, self.vcf, self.ranks[0].hh):
                    err = lib().bh_last_error().decode("utf-8", "replace")
                lib().bh_vcfstudy_close(self.vcfstudy)
                self.vcfstudy = C.c_void_p()
            if self.vcf:          # (every sample's file was renamed or removed when the sample ended)
                lib().bh_vcf_close(self.vcf)
                self.vcf = C.c_void_p()
            if self.cluster:      # (its tables were written when the sample was reported)
                lib().bh_cluster_close(self.cluster)
                self.cluster = C.c_void_p()
            if self.chimera:      # (likewise)
                lib().bh_chimera_close(self.chimera)
                self.chimera = C.c_void_p()
            lib().bh_session_close(self.h)
            self.h = C.c_void_p()
            if self.sam:      # (every sample's file was renamed or removed when the sample ended)
                lib().bh_sam_close(self.sam)
                self.sam = C.c_void_p()
            for i in range(len(self.ranks)):
                lib().bh_run_free(C.byref(self.ranks[i].run))
            if self.tax.n or self.tax.blob:
                lib().bh_tax_free(C.byref(self.tax))
            if err:
                raise HostError("tables not written: " + err)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


libc = C.CDLL(None)
libc.fopen.restype = C.c_void_p
libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [C.c_void_p]


SHARE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int)


def share_regions(off, part, n_parts, status, fetch, store, broadcast, any_failed, piece=64 << 20):
    """The exchange of the cooperative accelerator build (bhip_share_fn, include/burst_hip.h) over a launcher's own collectives, for ranks
    that have no RCCL communicator (the gloo back end; ranks sharing a device): region r of every rank's array, [off[r], off[r + 1]),
    travels from its builder to everybody, piece by piece through host memory.  fetch(a, n) -> bytes of the own array as a uint8 array,
    store(a, buf), broadcast(buf, root) -> buf, any_failed(status) -> bool.  Returns 0, 1 when some rank announced a failure before the
    exchange, -1 (on every rank) when a rank failed inside it."""
    if any_failed(status):
        return 1
    # A local failure in the middle (a device copy) must not leave the peers waiting in the next broadcast: the rank notes it, keeps
    # taking part with whatever buffer it has, and the ranks agree on the outcome in one more reduction at the end.
    broken = None
    for r in range(n_parts):
        a = int(off[r])
        while a < int(off[r + 1]):
            n = min(piece, int(off[r + 1]) - a)
            buf = np.empty(n, np.uint8)
            if r == part and broken is None:
                try:
                    buf = fetch(a, n)
                except Exception as e:
                    broken = e
            buf = broadcast(buf, r)
            if r != part and broken is None:
                try:
                    store(a, buf)
                except Exception as e:
                    broken = e
            a += n
    if broken is not None:
        sys.stderr.write("share_regions: rank %d: %s\n" % (part, broken))
    return -1 if any_failed(broken is not None) else 0


def dist_share(dist, pdev="cpu"):
    """bhip_share_fn over torch.distributed (any back end): returns the ctypes callback object for Db.open_device_shared -- the CALLER keeps
    it alive (a reference held) for as long as the library may call it, i.e. across bh_device_open_shared"""
    import torch
    def any_failed(status):
        t = torch.tensor([1 if status else 0], dtype=torch.int64, device=pdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(int(t.item()))
    def broadcast(buf, root):
        t = torch.from_numpy(buf).to(pdev)
        dist.broadcast(t, root)
        return t.cpu().numpy()
    class _Raw:          # a piece of the device array as a tensor, no copy (the nccl back end broadcasts it in place: RCCL over xGMI)
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    def cb(ctx, base, off, part, n_parts, status):
        try:
            if pdev != "cpu":
                if any_failed(status):
                    return 1
                for r in range(n_parts):
                    a = int(off[r])
                    while a < int(off[r + 1]):
                        n = min(1 << 30, int(off[r + 1]) - a)
                        dist.broadcast(torch.as_tensor(_Raw(base + a, n), device=pdev), r)
                        a += n
                torch.cuda.synchronize()
                return 0
            def fetch(a, n):
                out = np.empty(n, np.uint8)
                capi._chk(capi.lib().bhip_device_copy(out.ctypes.data, base + a, n, 0))
                return out
            def store(a, buf):
                buf = np.ascontiguousarray(buf)
                capi._chk(capi.lib().bhip_device_copy(base + a, buf.ctypes.data, len(buf), 1))
            return share_regions([off[i] for i in range(n_parts + 1)], part, n_parts, status, fetch, store, broadcast, any_failed)
        except Exception as e:          # (an exception must not unwind through the C caller)
            sys.stderr.write("dist_share: %s\n" % e)
            return -1
    return SHARE_FN(cb)


def shard_range(n_uniq, world, rank):
    """unique queries of rank `rank` of `world`: contiguous, sizes differing by at most one (a query and its reverse-complement twin
    are one unique query: they stay together)"""
    base, rem = divmod(n_uniq, world)
    u0 = rank * base + min(rank, rem)
    return u0, u0 + base + (1 if rank < rem else 0)


def clump_shard(db, world, rank):
    """clump range of database shard `rank` of `world` (bh_clump_shard: about the same number of reference columns each)"""
    c0, c1 = C.c_uint32(), C.c_uint32()
    lib().bh_clump_shard(C.byref(db.c), world, rank, C.byref(c0), C.byref(c1))
    return int(c0.value), int(c1.value)


def cigar_text(ops):
    """ops of one path (uint32 words length << 4 | code) as the report renders them (bh_cigar_text); raises on anything that is not an op"""
    ops = np.ascontiguousarray(ops, np.uint32)
    buf = C.create_string_buffer(12 * len(ops) + 2)
    n = lib().bh_cigar_text(ops.ctypes.data, len(ops), buf, len(buf))
    if not n:
        raise HostError("not a path: %r" % (ops.tolist(),))
    return buf.raw[:n].decode()


def report(path, db, qs, hits, mode, flags=0, cigar=None):
    """hits: HIT_DTYPE array with q = global entry index, records of one entry contiguous.  cigar: the capi.Device that holds the
    database -- every line then carries its path's position and CIGAR (bh_paths.c; bhip_trace_paths on that handle)"""
    f = libc.fopen(path.encode(), b"wb")
    if not f:
        raise HostError("cannot open %s" % path)
    n = C.c_uint64()
    hits = np.ascontiguousarray(hits)
    paths = C.c_void_p()
    try:
        if cigar is not None:
            _chk(lib().bh_paths_open(cigar._h, C.byref(paths)))
            view = BhRunView()
            view.base, view.n_runs, view.total = hits.ctypes.data, 1, len(hits)
            view.off[0], view.n[0] = 0, len(hits)
            _chk(lib().bh_report_view_paths(f, C.byref(db.c), C.byref(qs.c), C.byref(view), MODES[mode], flags, None, C.byref(n), None, paths))
        else:
            _chk(lib().bh_report_ex(f, C.byref(db.c), C.byref(qs.c), hits.ctypes.data_as(C.c_void_p), len(hits), MODES[mode], flags, C.byref(n)))
    finally:
        libc.fclose(f)
        if paths:
            lib().bh_paths_close(paths)
    return int(n.value)


def report_view(path, db, qs, view, mode, flags=0):
    """the same from a BhRunView (records in several runs: RankSearch.view)"""
    f = libc.fopen(path.encode(), b"wb")
    if not f:
        raise HostError("cannot open %s" % path)
    n = C.c_uint64()
    try:
        _chk(lib().bh_report_view(f, C.byref(db.c), C.byref(qs.c), C.byref(view), MODES[mode], flags, None, C.byref(n)))
    finally:
        libc.fclose(f)
    return int(n.value)


def synth_refs(path, n_base, n_variants, length, rate, seed, first_base=0):
    """base sequences [first_base, first_base + n_base) with their variants: a sequence depends on the seed and its number only"""
    _chk(lib().bh_synth_refs_range(path.encode(), first_base, n_base, n_variants, length, rate, seed))


def edx_merge(paths, out):
    """several .edx files laid end to end into one (bh_edx_merge)"""
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    _chk(lib().bh_edx_merge(arr, len(paths), out.encode()))


def synth_reads(refs, path, n_reads, read_len, edits, rc=False, iupac=0.0, seed=42, first_read=0, append=False):
    e = np.ascontiguousarray(edits, np.uint32)
    _chk(lib().bh_synth_reads_ex(refs.encode(), path.encode(), n_reads, read_len, e.ctypes.data_as(u32p), len(e), int(rc), iupac, seed, first_read, int(append)))


def dna_marks(sym, ref_start, ref_len, W, max_chain=0, max_sh=0):
    """the host restatement of one -d DNA partition's duplicate marks (bh_dna_marks_host): (flags, max_chain, max_sh)"""
    sym = np.ascontiguousarray(sym, np.uint8)
    rs = np.ascontiguousarray(ref_start, np.uint64)
    rl = np.ascontiguousarray(ref_len, np.uint32)
    flags = np.zeros(len(sym) + 1, np.uint8)
    mc, ms = C.c_uint64(max_chain), C.c_uint64(max_sh)
    _chk(lib().bh_dna_marks_host(sym.ctypes.data, rs.ctypes.data, rl.ctypes.data, len(rs), W, C.byref(mc), C.byref(ms), flags.ctypes.data))
    return flags[:len(sym)], mc.value, ms.value
