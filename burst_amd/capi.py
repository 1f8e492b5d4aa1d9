"""ctypes binding of libburst_hip.so (C ABI declared in include/burst_hip.h).

This is the only door from Python to the device path; there is no CPU fallback.  If the library has not
been built (`python -c "import __graft_entry__ as g; g.build()"` or `make -C burst_amd/csrc`) importing
this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BURST_AMD_LIBDIR: a directory with another build of the two libraries (tools/build_prof.sh: the phase-timer build)
LIB_PATH = os.path.join(os.environ.get("BURST_AMD_LIBDIR") or _HERE, "libburst_hip.so")

BHIP_OK, BHIP_E_ARG, BHIP_E_DEVICE, BHIP_E_CAPACITY, BHIP_E_QUERYLEN, BHIP_E_INTERNAL, BHIP_E_RESCORE = 0, -1, -2, -3, -4, -5, -6
BHIP_Q_PREFILTER, BHIP_Q_EXHAUSTIVE = 0, 1
BHIP_MAX_QLEN = 4095

# BhipHit, 20 bytes (include/burst_hip.h)
HIT_DTYPE = np.dtype([("q", "<u4"), ("refIx", "<u4"), ("finalPos", "<u4"), ("score", "<f4"),
                      ("ed", "u1"), ("gapR", "u1"), ("gapQ", "u1"), ("rc", "u1")])
assert HIT_DTYPE.itemsize == 20


class BhipStats(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_pairs", C.c_uint64), ("n_columns", C.c_uint64),
                ("n_raw_hits", C.c_uint64), ("n_hits", C.c_uint64), ("acx_entries_read", C.c_uint64),
                ("bytes_algorithmic", C.c_uint64), ("n_windows", C.c_uint64), ("n_window_columns", C.c_uint64),
                ("n_lane_tasks", C.c_uint64), ("n_task_columns", C.c_uint64), ("n_seed_words", C.c_uint64),
                ("ms_h2d", C.c_float), ("ms_prefilter", C.c_float), ("ms_peq", C.c_float), ("ms_myers", C.c_float),
                ("ms_rescore", C.c_float), ("ms_d2h", C.c_float), ("ms_total", C.c_float),
                ("ms_myers_prefix", C.c_float), ("ms_myers_window", C.c_float), ("ms_prefilter_hash", C.c_float), ("ms_seed", C.c_float),
                ("ms_stage_copy", C.c_float), ("ms_stage_route", C.c_float),
                ("myers_launches", C.c_uint32), ("prefix_words", C.c_uint32), ("prefilter_launches", C.c_uint32), ("prefilter_algo", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BhipQuerySpan(C.Structure):
    _fields_ = [("codes", C.c_void_p), ("codes4", C.c_void_p), ("off", C.c_void_p), ("emac", C.c_void_p), ("rc", C.c_void_p), ("flags", C.c_void_p),
                ("n", C.c_uint32), ("q_base", C.c_uint32), ("codes2", C.c_void_p), ("len", C.c_void_p)]


EXPORTS = ["bhip_init", "bhip_stage_queries", "bhip_align_staged", "bhip_align_batch", "bhip_align_pairs", "bhip_prefilter", "bhip_set_option", "bhip_get_stats",
           "bhip_device_info", "bhip_destroy", "bhip_last_error", "bhip_abi_version", "bhip_set_ref_order", "bhip_copy_hits_device", "bhip_sync_hits",
           "bhip_comm_create", "bhip_comm_unique_id", "bhip_comm_create_rank", "bhip_comm_allreduce_min", "bhip_comm_fetch_gathered", "bhip_comm_gather_hits", "bhip_comm_stage_device", "bhip_comm_gather_staged", "bhip_comm_stage_reset", "bhip_comm_destroy", "bhip_acx_export", "bhip_reserve", "bhip_reserve_symbols", "bhip_sort_queries", "bhip_stage_spans", "bhip_alloc_host", "bhip_free_host", "bhip_host_register", "bhip_host_unregister", "bhip_set_enqueued_hook", "bhip_acx_export_entries",
           "bhip_build_accelerator_shared", "bhip_comm_share", "bhip_team_create", "bhip_team_destroy", "bhip_team_share", "bhip_device_copy", "bhip_dna_marks",
           "bhip_cov_begin", "bhip_cov_add", "bhip_cov_sample_stats", "bhip_cov_dataset_stats", "bhip_cov_info", "bhip_cov_end", "bhip_lane_extents",
           "bhip_trace_paths", "bhip_paths_info", "bhip_mates_join", "bhip_mates_info", "bhip_em_run", "bhip_taxa_run", "bhip_taxa_rollup", "bhip_pile_run", "bhip_consensus_run", "bhip_consensus_info",
           "bhip_consensus_pairs", "bhip_consensus_pairs_info",
           "bhip_alleles_run", "bhip_alleles_info", "bhip_site_counts", "bhip_site_counts_info",
           "bhip_cluster_run", "bhip_cluster_info", "bhip_chimera_run", "bhip_chimera_info", "bhip_md_tags"]

# BhipMateLine, 20 bytes: pair and header numbers, .b6 columns 9 and 10 (signed), column 11
MATE_LINE_DTYPE = np.dtype([("pair", "<u4"), ("ref", "<u4"), ("st", "<i4"), ("ed", "<i4"), ("edits", "<u4")])
assert MATE_LINE_DTYPE.itemsize == 20
MATES_FR, MATES_RF, MATES_FF = 0, 1, 2
MATES_ALL, MATES_BEST = 0, 1
MATES_ORIENTATIONS = {"fr": MATES_FR, "rf": MATES_RF, "ff": MATES_FF}
MATES_REPORTS = {"all": MATES_ALL, "best": MATES_BEST}

# BhipPathReq, 16 bytes: query entry, refIx, finalPos, ed of a record
PATH_REQ_DTYPE = np.dtype([("q", "<u4"), ("refIx", "<u4"), ("finalPos", "<u4"), ("ed", "<u4")])
assert PATH_REQ_DTYPE.itemsize == 16
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OP_CHARS = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def cigar_text(ops):
    """ops of one path (words length << 4 | code) as CIGAR text in =XID"""
    return "".join("%d%s" % (int(w) >> 4, OP_CHARS[int(w) & 15]) for w in ops)


# BhipCovLine, 16 bytes: header, .b6 columns 9 and 10, weight (bits 0..30) | unique << 31
COV_LINE_DTYPE = np.dtype([("ref", "<u4"), ("st", "<u4"), ("ed", "<u4"), ("w", "<u4")])
assert COV_LINE_DTYPE.itemsize == 16


# BhipEmLine, 8 bytes: group and header numbers of one printed line (bhip_em_run)
EM_LINE_DTYPE = np.dtype([("group", "<u4"), ("ref", "<u4")])
assert EM_LINE_DTYPE.itemsize == 8


# BhipPileLine, 40 bytes: a path (query entry, lane, first lane column, its ops) placed on a header at a position, for w reads (bhip_pile_run)
PILE_LINE_DTYPE = np.dtype({"names": ["q", "refIx", "ref_first", "header", "pos", "w", "n_ops", "op_off"], "formats": ["<u4"] * 7 + ["<u8"],
                            "offsets": [0, 4, 8, 12, 16, 20, 24, 32], "itemsize": 40})
# BhipPileSite, 44 bytes: header, position, reference code, depth, the reads per class (A C G T Del Other), insertion marks
PILE_SITE_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("ref", "<u4"), ("depth", "<u4"), ("n", "<u4", (6,)), ("ins", "<u4")])
assert PILE_LINE_DTYPE.itemsize == 40 and PILE_SITE_DTYPE.itemsize == 44
PILE_INFO = ("events", "candidates", "sites", "device_us", "peak_bytes")
# BhipConsSeg, 48 bytes: a maximal run of covered positions of a header, its figures, and where its letters start (bhip_consensus_run)
CONS_SEG_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("len", "<u4"), ("called", "<u4"), ("same", "<u4"), ("subst", "<u4"), ("del", "<u4"), ("ambig", "<u4"),
                           ("ins_major", "<u4"), ("pad", "<u4"), ("off", "<u8")])
assert CONS_SEG_DTYPE.itemsize == 48
CONS_INFO = ("events", "candidates", "segments", "covered", "device_us", "peak_bytes")
# bhip_consensus_pairs: BhipPairSeg, 24 bytes: a segment of a sample's consensus row on a header and where its letters start; BhipPair, 24 bytes:
# samples a < b on a header, the positions comparable in both rows and those of them with equal letters
PAIR_SEG_DTYPE = np.dtype([("sample", "<u4"), ("header", "<u4"), ("pos", "<u4"), ("len", "<u4"), ("off", "<u8")])
PAIR_DTYPE = np.dtype([("header", "<u4"), ("a", "<u4"), ("b", "<u4"), ("pad", "<u4"), ("compared", "<u4"), ("same", "<u4")])
assert PAIR_SEG_DTYPE.itemsize == 24 and PAIR_DTYPE.itemsize == 24
CONS_PAIRS_INFO = ("segments", "headers", "union_positions", "examined", "pairs", "device_us", "peak_bytes")


def pair_arrays(segs, letters):
    """the two inputs of consensus_pairs as contiguous arrays (segs: PAIR_SEG_DTYPE or rows of it; letters: bytes, str or uint8)"""
    segs = np.zeros(0, PAIR_SEG_DTYPE) if segs is None or len(segs) == 0 else np.ascontiguousarray(segs, dtype=PAIR_SEG_DTYPE)
    if isinstance(letters, str):
        letters = letters.encode()
    letters = np.frombuffer(letters, np.uint8) if isinstance(letters, (bytes, bytearray)) else np.ascontiguousarray(letters, dtype=np.uint8)
    return segs, letters
# BhipAllele, 40 bytes: an indel allele behind the anchor (header, pos) (bhip_alleles_run).  allele: Del(n) = n; Ins = n << 60 | c1 << 56 | ...
ALLELE_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("allele", "<u8"), ("ref", "<u4"), ("depth", "<u4"), ("count", "<u4"), ("pad", "<u4"), ("code_off", "<u8")])
assert ALLELE_DTYPE.itemsize == 40
ALLELES_INFO = ("events", "distinct", "alleles", "skipped_end", "skipped_adjacent", "skipped_long", "device_us", "peak_bytes")
# bhip_site_counts: BhipCountRange, 16 bytes: a line covers [pos, pos + span - 1] of a header for w reads; BhipCountRecord, 24 bytes: allele 0 = a
# site record (ref 1..4), else the allele word; BhipCountCell, 24 bytes: depth, n[A C G T], count
COUNT_RANGE_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("span", "<u4"), ("w", "<u4")])
COUNT_RECORD_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("allele", "<u8"), ("ref", "<u4"), ("pad", "<u4")])
COUNT_CELL_DTYPE = np.dtype([("depth", "<u4"), ("n", "<u4", (4,)), ("count", "<u4")])
assert COUNT_RANGE_DTYPE.itemsize == 16 and COUNT_RECORD_DTYPE.itemsize == 24 and COUNT_CELL_DTYPE.itemsize == 24
SITE_COUNTS_INFO = ("ranges", "records", "device_us", "peak_bytes")
MD_INFO = ("device_us", "requests", "md_bytes", "peak_bytes")

# BhipClusterEdge, 12 bytes: read q has a printed line against read r with this many edits (bhip_cluster_run)
CLUSTER_EDGE_DTYPE = np.dtype([("q", "<u4"), ("r", "<u4"), ("edits", "<u4")])
assert CLUSTER_EDGE_DTYPE.itemsize == 12
CLUSTER_INFO = ("rounds", "edges_kept", "centroids", "device_us", "device_bytes", "edges", "nodes")


def count_arrays(ranges, sites, alleles, records):
    """the four inputs of site_counts as contiguous arrays of their dtypes (None or an empty list: none)"""
    def arr(x, dt):
        return np.zeros(0, dt) if x is None or len(x) == 0 else np.ascontiguousarray(x, dtype=dt)
    return arr(ranges, COUNT_RANGE_DTYPE), arr(sites, PILE_SITE_DTYPE), arr(alleles, ALLELE_DTYPE), arr(records, COUNT_RECORD_DTYPE)


def cluster_edges(rows):
    """a CLUSTER_EDGE_DTYPE array as it is (contiguous), rows (q, r, edits) as one"""
    if isinstance(rows, np.ndarray) and rows.dtype == CLUSTER_EDGE_DTYPE:
        return np.ascontiguousarray(rows)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(rows), CLUSTER_EDGE_DTYPE)
    out["q"], out["r"], out["edits"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return out


# BhipChimLine, 24 bytes: read q has a printed line against read r (flags bit 0: reverse strand) with the path ops[op_off : op_off + n_ops];
# BhipChimera, 32 bytes: a read's row (bhip_chimera_run)
CHIM_LINE_DTYPE = np.dtype([("q", "<u4"), ("r", "<u4"), ("flags", "<u4"), ("n_ops", "<u4"), ("op_off", "<u8")])
CHIMERA_DTYPE = np.dtype([("role", "<u4"), ("single", "<u4"), ("model", "<u4"), ("cut", "<u4"), ("a", "<u4"), ("ea", "<u4"), ("b", "<u4"), ("eb", "<u4")])
assert CHIM_LINE_DTYPE.itemsize == 24 and CHIMERA_DTYPE.itemsize == 32
CHIMERA_INFO = ("pairs_kept", "evaluated", "chimeric", "device_us", "device_bytes", "lines", "nodes")


def chim_lines(rows):
    """a CHIM_LINE_DTYPE array as it is (contiguous), rows (q, r, flags, n_ops, op_off) as one"""
    if isinstance(rows, np.ndarray) and rows.dtype == CHIM_LINE_DTYPE:
        return np.ascontiguousarray(rows)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    out = np.zeros(len(rows), CHIM_LINE_DTYPE)
    out["q"], out["r"], out["flags"], out["n_ops"], out["op_off"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
    return out


def pile_lines(rows):
    """a PILE_LINE_DTYPE array as it is (contiguous), rows (q, refIx, ref_first, header, pos, w, n_ops, op_off) as one"""
    if isinstance(rows, np.ndarray) and rows.dtype == PILE_LINE_DTYPE:
        return np.ascontiguousarray(rows)
    if isinstance(rows, np.ndarray) and rows.dtype.names == PILE_LINE_DTYPE.names:      # (the same fields without the padding: numpy packs what it concatenates)
        out = np.zeros(len(rows), PILE_LINE_DTYPE)
        for name in PILE_LINE_DTYPE.names:
            out[name] = rows[name]
        return out
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 8)
    out = np.zeros(len(rows), PILE_LINE_DTYPE)
    for k, name in enumerate(PILE_LINE_DTYPE.names):
        out[name] = rows[:, k]
    return out


def em_lines(rows):
    """an EM_LINE_DTYPE array as it is, rows (group, ref) as one"""
    if isinstance(rows, np.ndarray) and rows.dtype == EM_LINE_DTYPE:
        return np.ascontiguousarray(rows)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(rows), EM_LINE_DTYPE)
    out["group"], out["ref"] = rows[:, 0], rows[:, 1]
    return out


def _mate_lines(rows):
    """rows (pair, ref, st, ed, edits) as a MATE_LINE_DTYPE array"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    out = np.zeros(len(rows), MATE_LINE_DTYPE)
    for k, name in enumerate(MATE_LINE_DTYPE.names):
        out[name] = rows[:, k]
    return out


class BurstHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libburst_hip error %d: %s" % (code, msg))
        self.code = code


LOAD_LEGACY_PREFILTERS = False


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: the HIP extension has not been built (run __graft_entry__.build()); "
                          "burst_amd has no CPU fallback" % LIB_PATH)
    # The superseded prefilter kernels (options prefilter_cw = 0 / 1) are NOT in libburst_hip.so: the tests ask for the test-only library
    # that holds them (tests/conftest.py sets LOAD_LEGACY_PREFILTERS in THIS process; child processes -- bench.py, burst_hip -- run the
    # product library alone).  Loaded first and globally, so that the product library's weak reference (bhip_internal.h:
    # bhip_legacy_pf_kernel) resolves to it.
    legacy = os.path.join(os.path.dirname(LIB_PATH), "libburst_hip_legacy.so")
    if LOAD_LEGACY_PREFILTERS and os.path.exists(legacy):
        globals()["_legacy_lib"] = C.CDLL(legacy, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    lib.bhip_init.argtypes = [i32, vp, vp, u32, u32, vp, vp, i32, i32, vp, u32, vp, i32, C.POINTER(vp)]
    lib.bhip_init.restype = i32
    lib.bhip_dna_marks.argtypes = [i32, vp, u64, vp, vp, u64, u32, C.POINTER(u64), C.POINTER(u64), vp, vp]
    lib.bhip_dna_marks.restype = i32
    lib.bhip_align_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, vp, u64, C.POINTER(u64)]
    lib.bhip_align_batch.restype = i32
    lib.bhip_stage_queries.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32]
    lib.bhip_stage_queries.restype = i32
    lib.bhip_align_staged.argtypes = [vp, i32, vp, u64, C.POINTER(u64)]
    lib.bhip_align_staged.restype = i32
    lib.bhip_align_pairs.argtypes = [vp, vp, vp, vp, u32, vp, vp, u64, vp]
    lib.bhip_align_pairs.restype = i32
    lib.bhip_prefilter.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u64, C.POINTER(u64)]
    lib.bhip_prefilter.restype = i32
    lib.bhip_set_option.argtypes = [vp, C.c_char_p, C.c_longlong]
    lib.bhip_set_option.restype = i32
    lib.bhip_get_stats.argtypes = [vp, C.POINTER(BhipStats)]
    lib.bhip_get_stats.restype = i32
    lib.bhip_device_info.argtypes = [vp, C.c_char_p, i32, C.POINTER(i32), C.POINTER(u64)]
    lib.bhip_device_info.restype = i32
    lib.bhip_copy_hits_device.argtypes = [vp, vp, u64, C.POINTER(u64)]
    lib.bhip_copy_hits_device.restype = i32
    lib.bhip_sync_hits.argtypes = [vp]
    lib.bhip_sync_hits.restype = i32
    lib.bhip_destroy.argtypes = [vp]
    lib.bhip_destroy.restype = None
    lib.bhip_last_error.argtypes = []
    lib.bhip_last_error.restype = C.c_char_p
    lib.bhip_set_ref_order.argtypes = [vp, vp, u32]
    lib.bhip_set_ref_order.restype = i32
    lib.bhip_abi_version.argtypes = []
    lib.bhip_abi_version.restype = i32
    lib.bhip_stage_spans.argtypes = [vp, C.POINTER(BhipQuerySpan), u32, u32, u32]
    lib.bhip_reserve.argtypes = [vp, u32, u32]
    lib.bhip_reserve.restype = i32
    lib.bhip_stage_spans.restype = i32
    lib.bhip_reserve_symbols.argtypes = [vp, u32, u32, u64]
    lib.bhip_reserve_symbols.restype = i32
    lib.bhip_alloc_host.argtypes = [u64]
    lib.bhip_alloc_host.restype = vp
    lib.bhip_free_host.argtypes = [vp]
    lib.bhip_free_host.restype = None
    lib.bhip_host_register.argtypes = [vp, u64]
    lib.bhip_host_register.restype = i32
    lib.bhip_host_unregister.argtypes = [vp]
    lib.bhip_host_unregister.restype = i32
    lib.bhip_comm_unique_id.argtypes = [vp]
    lib.bhip_comm_unique_id.restype = i32
    lib.bhip_comm_create_rank.argtypes = [i32, i32, i32, vp, C.POINTER(vp)]
    lib.bhip_comm_create_rank.restype = i32
    lib.bhip_comm_destroy.argtypes = [vp]
    lib.bhip_comm_destroy.restype = None
    lib.bhip_acx_export.argtypes = [vp, vp, vp, vp, u64, C.POINTER(u64), vp, u32, C.POINTER(u32)]
    lib.bhip_acx_export.restype = i32
    lib.bhip_build_accelerator_shared.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.bhip_build_accelerator_shared.restype = i32
    lib.bhip_team_create.argtypes = [i32, C.POINTER(vp)]
    lib.bhip_team_create.restype = i32
    lib.bhip_team_destroy.argtypes = [vp]
    lib.bhip_team_destroy.restype = None
    lib.bhip_device_copy.argtypes = [vp, vp, u64, i32]
    lib.bhip_device_copy.restype = i32
    lib.bhip_cov_begin.argtypes = [vp, u32, vp, u32]
    lib.bhip_cov_add.argtypes = [vp, u32, vp, u64]
    lib.bhip_cov_sample_stats.argtypes = [vp, u32, vp, vp]
    lib.bhip_cov_dataset_stats.argtypes = [vp, vp, vp]
    lib.bhip_cov_info.argtypes = [vp, vp]
    lib.bhip_cov_end.argtypes = [vp]
    lib.bhip_lane_extents.argtypes = [vp, vp]
    lib.bhip_trace_paths.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, vp, vp, vp]
    lib.bhip_trace_paths.restype = i32
    lib.bhip_paths_info.argtypes = [vp, vp]
    lib.bhip_paths_info.restype = i32
    lib.bhip_mates_join.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32, u32, vp, vp, u64, C.POINTER(u64)]
    lib.bhip_mates_join.restype = i32
    lib.bhip_mates_info.argtypes = [vp, vp]
    lib.bhip_mates_info.restype = i32
    lib.bhip_em_run.argtypes = [vp, u32, u32, vp, vp, u64, u32, u64, vp, vp]
    lib.bhip_em_run.restype = i32
    lib.bhip_taxa_run.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, u64, u32, vp, vp, vp, vp]
    lib.bhip_taxa_run.restype = i32
    lib.bhip_taxa_rollup.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
    lib.bhip_taxa_rollup.restype = i32
    lib.bhip_pile_run.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, u32, u32, vp, u64, C.POINTER(u64), vp]
    lib.bhip_pile_run.restype = i32
    lib.bhip_consensus_run.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp]
    lib.bhip_consensus_run.restype = i32
    lib.bhip_consensus_info.argtypes = [vp, vp]
    lib.bhip_consensus_info.restype = i32
    lib.bhip_consensus_pairs.argtypes = [vp, u32, vp, u64, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    lib.bhip_consensus_pairs.restype = i32
    lib.bhip_consensus_pairs_info.argtypes = [vp, vp]
    lib.bhip_consensus_pairs_info.restype = i32
    lib.bhip_alleles_run.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, u32, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), vp]
    lib.bhip_alleles_run.restype = i32
    lib.bhip_alleles_info.argtypes = [vp, vp]
    lib.bhip_alleles_info.restype = i32
    lib.bhip_site_counts.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp]
    lib.bhip_site_counts.restype = i32
    lib.bhip_site_counts_info.argtypes = [vp, vp]
    lib.bhip_site_counts_info.restype = i32
    lib.bhip_cluster_run.argtypes = [vp, u32, vp, vp, u64, vp, vp]
    lib.bhip_cluster_run.restype = i32
    lib.bhip_cluster_info.argtypes = [vp, vp]
    lib.bhip_cluster_info.restype = i32
    lib.bhip_chimera_run.argtypes = [vp, u32, vp, vp, vp, u64, vp, u64, u32, u32, u32, vp]
    lib.bhip_chimera_run.restype = i32
    lib.bhip_chimera_info.argtypes = [vp, vp]
    lib.bhip_chimera_info.restype = i32
    lib.bhip_md_tags.argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp]
    lib.bhip_md_tags.restype = i32
    for f in (lib.bhip_cov_begin, lib.bhip_cov_add, lib.bhip_cov_sample_stats, lib.bhip_cov_dataset_stats, lib.bhip_cov_info, lib.bhip_cov_end, lib.bhip_lane_extents):
        f.restype = i32
    return lib


_lib = None


def _hits_mode(all_hits):
    """False / True (every hit within budget) as before; 2 or "best" = BHIP_HITS_BEST (one record per entry, chosen on the device)"""
    return 2 if all_hits in (2, "best") else int(bool(all_hits))


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _chk(rc):
    if rc != BHIP_OK:
        raise BurstHipError(rc, lib().bhip_last_error().decode("utf-8", "replace"))


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


class Queries:
    """Flat query batch in the layout bhip_align_batch takes."""

    def __init__(self, seqs, emac, six=None, rc=None, flags=None):
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        self.off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=self.off[1:])
        self.codes = (np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if len(seqs) and self.off[-1]
                      else np.zeros(1, np.uint8))
        self.emac = _arr(emac, np.uint16)
        self.six = _arr(six, np.uint32)
        self.rc = _arr(rc, np.uint8)
        self.flags = _arr(flags, np.uint8)
        self.n = len(seqs)
        self.n_shared = int(self.six.max()) + 1 if self.six is not None and self.n else self.n


class Device:
    """One handle = one database resident on one GPU (bhip_init .. bhip_destroy)."""

    def __init__(self, edx_packed, clump_len, tot_refs, score_lut, acx_lens=None, acx_lists=None, acx_fmt=0, K=12,
                 badlist=None, device=0, xalpha=0, build_acx=False):
        """acx_lens / acx_lists: the tables of an .acx file; build_acx=True (and no tables): the device builds the accelerator
        for word length K from the references alone"""
        self._h = C.c_void_p()
        if acx_lens is None and not build_acx:
            K = 0
        edx_packed = _arr(edx_packed, np.uint8)
        clump_len = _arr(clump_len, np.uint32)
        score_lut = _arr(score_lut, np.uint8)
        acx_lens = _arr(acx_lens, np.uint32)
        acx_lists = _arr(acx_lists, np.uint8)
        badlist = _arr(badlist, np.uint32)
        nbad = 0 if badlist is None else len(badlist)
        self.n_clumps = len(clump_len)
        self.clump_len = clump_len
        _chk(lib().bhip_init(device, _ptr(edx_packed), _ptr(clump_len), len(clump_len), tot_refs, _ptr(acx_lens), _ptr(acx_lists),
                             acx_fmt, K, _ptr(badlist), nbad, _ptr(score_lut), xalpha, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().bhip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int()
        hbm = C.c_uint64()
        _chk(lib().bhip_device_info(self._h, name, 256, C.byref(ncu), C.byref(hbm)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": hbm.value}

    def acx_export(self, K, masks=True):
        """the handle's accelerator in the file's terms: (Lens[4^K], clump ids in word order, lane masks or None, BadList)"""
        n, nb = C.c_uint64(), C.c_uint32()
        _chk(lib().bhip_acx_export(self._h, None, None, None, 0, C.byref(n), None, 0, C.byref(nb)))
        lens = np.zeros(1 << (2 * K), np.uint32)
        clumps = np.zeros(max(1, n.value), np.uint32)
        mk = np.zeros(max(1, n.value), np.uint16) if masks else None
        bad = np.zeros(max(1, nb.value), np.uint32)
        _chk(lib().bhip_acx_export(self._h, _ptr(lens), _ptr(clumps), _ptr(mk), n.value, C.byref(n), _ptr(bad), nb.value, C.byref(nb)))
        return lens, clumps[:n.value], (mk[:n.value] if masks else None), bad[:nb.value]

    def set_option(self, name, value):
        _chk(lib().bhip_set_option(self._h, name.encode(), int(value)))

    def reserve(self, n_entries, max_len):
        """bhip_reserve: size the device buffers for batches of n_entries query entries of at most max_len symbols and run the
        library's warm-up pass (what the burst_hip command line does once per job, before the search phase)"""
        _chk(lib().bhip_reserve(self._h, int(n_entries), int(max_len)))

    def stats(self, raw=False):
        """statistics of the last call (raw=True: the ctypes struct, no dict -- for timed loops)"""
        s = BhipStats()
        _chk(lib().bhip_get_stats(self._h, C.byref(s)))
        return s if raw else s.as_dict()

    def set_ref_order(self, order):
        """BEST's tie-break table (order[refIx] = RefIxSrt[refIx]) for all_hits = 2 / "best" (bhip_set_ref_order)"""
        order = _arr(order, np.uint32)
        _chk(lib().bhip_set_ref_order(self._h, _ptr(order), len(order)))

    def align_batch(self, q, all_hits=False, cap=None):
        cap = cap or max(1 << 16, 4 * q.n)
        while True:
            hits = np.zeros(cap, dtype=HIT_DTYPE)
            n = C.c_uint64()
            rc = lib().bhip_align_batch(self._h, _ptr(q.codes), _ptr(q.off), _ptr(q.emac), _ptr(q.six), _ptr(q.rc), _ptr(q.flags),
                                        q.n, q.n_shared, _hits_mode(all_hits), _ptr(hits), cap, C.byref(n))
            if rc == BHIP_E_CAPACITY:
                cap = int(n.value) + 16
                continue
            _chk(rc)
            return hits[:n.value]

    def stage(self, q):
        """upload a batch once (bhip_stage_queries); align_staged() then runs on the resident copy"""
        self._staged = q     # keep the host arrays alive
        _chk(lib().bhip_stage_queries(self._h, _ptr(q.codes), _ptr(q.off), _ptr(q.emac), _ptr(q.six), _ptr(q.rc), _ptr(q.flags), q.n, q.n_shared))

    def stage_spans(self, spans, n_shared, max_len=0):
        """asynchronous staging (bhip_stage_spans).  spans: list of dicts with numpy arrays codes, off (n + 1 offsets into codes),
        emac and optional rc / flags, plus q_base; entry j of every span shares slot j.  The arrays are kept alive here until
        the next two batches have been staged (the library reads them until the batch has been aligned)."""
        arr = (BhipQuerySpan * max(1, len(spans)))()
        keep = []
        n_tot = 0
        for k, sp in enumerate(spans):
            codes, off, emac = _arr(sp["codes"], np.uint8), _arr(sp["off"], np.uint64), _arr(sp["emac"], np.uint16)
            rc, fl = _arr(sp.get("rc"), np.uint8), _arr(sp.get("flags"), np.uint8)
            keep += [codes, off, emac, rc, fl]
            n = len(off) - 1
            arr[k].codes, arr[k].off, arr[k].emac = codes.ctypes.data, off.ctypes.data, emac.ctypes.data
            c4 = _arr(sp.get("codes4"), np.uint8)
            keep.append(c4)
            arr[k].codes4 = c4.ctypes.data if c4 is not None else None
            arr[k].rc = rc.ctypes.data if rc is not None else None
            arr[k].flags = fl.ctypes.data if fl is not None else None
            arr[k].n, arr[k].q_base = n, int(sp.get("q_base", 0))
            c2, ln = _arr(sp.get("codes2"), np.uint8), _arr(sp.get("len"), np.uint16)
            keep += [c2, ln]
            arr[k].codes2 = c2.ctypes.data if c2 is not None else None
            arr[k].len = ln.ctypes.data if ln is not None else None
            n_tot += n
        self._span_keep = getattr(self, "_span_keep", [])[-2:] + [keep]
        self._staged_n = n_tot
        _chk(lib().bhip_stage_spans(self._h, arr, len(spans), int(n_shared), int(max_len)))

    def align_staged(self, all_hits=False, out=None):
        """out: optional preallocated HIT_DTYPE array reused between calls"""
        hits = out if out is not None else np.zeros(max(1 << 16, 4 * (self._staged.n if getattr(self, "_staged", None) is not None else getattr(self, "_staged_n", 0))), dtype=HIT_DTYPE)
        while True:
            n = C.c_uint64()
            rc = lib().bhip_align_staged(self._h, _hits_mode(all_hits), _ptr(hits), len(hits), C.byref(n))
            if rc == BHIP_E_CAPACITY:
                hits = np.zeros(int(n.value) + 16, dtype=HIT_DTYPE)
                continue
            _chk(rc)
            return hits[:n.value], hits

    def sync_hits(self):
        """with option async_d2h: wait until the records of the previous calls are in their host buffers"""
        _chk(lib().bhip_sync_hits(self._h))

    def copy_hits_device(self, dst_ptr, cap_records):
        """device-to-device copy of the last call's records into caller-owned device memory (e.g. a torch tensor's data_ptr())"""
        n = C.c_uint64()
        _chk(lib().bhip_copy_hits_device(self._h, C.c_void_p(int(dst_ptr)), int(cap_records), C.byref(n)))
        return int(n.value)

    def lane_extents(self):
        """index after the last non-pad symbol of every lane of the resident database, [16 * clump + lane] (bhip_lane_extents)"""
        ext = np.zeros(16 * self.n_clumps, np.uint32)
        _chk(lib().bhip_lane_extents(self._h, _ptr(ext)))
        return ext

    def trace_paths(self, q, requests, cap=None):
        """alignment paths of records (bhip_trace_paths).  q: the Queries the records' entry numbers refer to; requests: PATH_REQ_DTYPE array
        (or rows q, refIx, finalPos, ed).  Returns (ops, op_off, ref_first, gap_r): request i owns ops[op_off[i]:op_off[i + 1]]"""
        if not (isinstance(requests, np.ndarray) and requests.dtype == PATH_REQ_DTYPE):
            rows = np.asarray(requests, dtype=np.uint32).reshape(-1, 4)
            requests = np.zeros(len(rows), PATH_REQ_DTYPE)
            for k, name in enumerate(("q", "refIx", "finalPos", "ed")):
                requests[name] = rows[:, k]
        requests = np.ascontiguousarray(requests)
        n = len(requests)
        cap = int(cap) if cap is not None else max(16, 4 * n)
        op_off = np.zeros(n + 1, np.uint64)
        ref_first, gap_r = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        while True:
            ops = np.zeros(max(cap, 1), np.uint32)
            rc = lib().bhip_trace_paths(self._h, _ptr(q.codes), _ptr(q.off), q.n, _ptr(requests), n, _ptr(ops), cap, _ptr(op_off), _ptr(ref_first), _ptr(gap_r))
            if rc == BHIP_E_CAPACITY and int(op_off[n]) > cap:
                cap = int(op_off[n])
                continue
            _chk(rc)
            return ops[:int(op_off[n])], op_off, ref_first[:n], gap_r[:n]

    def paths_info(self):
        info = np.zeros(4, np.uint64)
        _chk(lib().bhip_paths_info(self._h, _ptr(info)))
        return dict(zip(("us_last", "us_total", "requests", "ops"), (int(x) for x in info)))

    def mates_join(self, a, b, orientation="fr", ins_min=0, ins_max=1000, report="all", cap=None):
        """concordant combinations of two mates' lines (bhip_mates_join).  a, b: MATE_LINE_DTYPE arrays (or rows pair, ref, st, ed, edits);
        orientation fr / rf / ff and report all / best by name or number.  Returns (out_a, out_b): indices into a and b, ascending (a, b).
        cap: room offered at first (default: one combination per line of a); a capacity answer is retried once with the wanted room"""
        a, b = (x if isinstance(x, np.ndarray) and x.dtype == MATE_LINE_DTYPE else _mate_lines(x) for x in (a, b))
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        orientation = MATES_ORIENTATIONS.get(orientation, orientation)
        report = MATES_REPORTS.get(report, report)
        cap = len(a) if cap is None else int(cap)
        n = C.c_uint64(0)
        for _ in range(2):
            out_a, out_b = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
            rc = lib().bhip_mates_join(self._h, _ptr(a), len(a), _ptr(b), len(b), int(orientation), int(ins_min), int(ins_max), int(report),
                                       _ptr(out_a), _ptr(out_b), cap, C.byref(n))
            if rc != BHIP_E_CAPACITY or n.value <= cap:
                break
            cap = n.value
        _chk(rc)
        return out_a[:n.value], out_b[:n.value]

    def mates_info(self):
        info = np.zeros(4, np.uint64)
        _chk(lib().bhip_mates_info(self._h, _ptr(info)))
        return dict(zip(("us_last", "us_total", "lines", "combinations"), (int(x) for x in info)))

    def taxa_run(self, parent, header_node, group_w, lines, agree=1000):
        """the taxa of one sample's groups (bhip_taxa_run): parent[v] of a tree numbered in preorder, header_node[h], group_w[g] = reads of group
        g, lines: EM_LINE_DTYPE array (or rows group, ref), agree in permille.  Returns (group_node uint32 [groups], 0xFFFFFFFF = no lines;
        own, clade uint64 [nodes]; info uint64 [8]: pairs, groups with lines, their reads, reads at the root, deepest level, device
        microseconds, peak device bytes, 0)"""
        parent, header_node = np.ascontiguousarray(parent, dtype=np.uint32), np.ascontiguousarray(header_node, dtype=np.uint32)
        group_w = np.ascontiguousarray(group_w, dtype=np.uint32)
        lines = em_lines(lines)
        nn = len(parent)
        gn, own, clade, info = np.zeros(max(len(group_w), 1), np.uint32), np.zeros(max(nn, 1), np.uint64), np.zeros(max(nn, 1), np.uint64), np.zeros(8, np.uint64)
        _chk(lib().bhip_taxa_run(self._h, nn, _ptr(parent), len(header_node), _ptr(header_node), len(group_w), _ptr(group_w), _ptr(lines), len(lines), int(agree),
                                 _ptr(gn), _ptr(own), _ptr(clade), _ptr(info)))
        return gn[:len(group_w)], own[:nn], clade[:nn], info

    def taxa_rollup(self, parent, header_node, header_count):
        """counts per header summed per node and per subtree (bhip_taxa_rollup): (own, clade) uint64 [nodes]"""
        parent, header_node = np.ascontiguousarray(parent, dtype=np.uint32), np.ascontiguousarray(header_node, dtype=np.uint32)
        header_count = np.ascontiguousarray(header_count, dtype=np.uint64)
        nn = len(parent)
        own, clade = np.zeros(max(nn, 1), np.uint64), np.zeros(max(nn, 1), np.uint64)
        _chk(lib().bhip_taxa_rollup(self._h, nn, _ptr(parent), len(header_node), _ptr(header_node), _ptr(header_count), _ptr(own), _ptr(clade)))
        return own[:nn], clade[:nn]

    def em_run(self, n_headers, group_w, lines, max_iters=1000, tol=1024):
        """abundance of one sample (bhip_em_run): group_w[g] = reads of group g, lines: EM_LINE_DTYPE array (or rows group, ref).  Returns
        (counts uint64 [n_headers] in units of 2^-30 read, info uint64 [8]: iterations, pairs, classes, last delta, stopped on tol, device
        microseconds, peak device bytes, 0)"""
        group_w = np.ascontiguousarray(group_w, dtype=np.uint32)
        lines = em_lines(lines)
        counts, info = np.zeros(max(int(n_headers), 1), np.uint64), np.zeros(8, np.uint64)
        _chk(lib().bhip_em_run(self._h, int(n_headers), len(group_w), _ptr(group_w), _ptr(lines), len(lines), int(max_iters), int(tol), _ptr(counts), _ptr(info)))
        return counts[:int(n_headers)], info

    def pile_run(self, q, lines, ops, min_depth=4, min_alt=2, cap=None):
        """variant sites of one sample (bhip_pile_run).  q: the Queries the lines' entry numbers refer to; lines: PILE_LINE_DTYPE array (or
        rows q, refIx, ref_first, header, pos, w, n_ops, op_off); ops: the uint32 op words the lines point into.  Returns the sites
        (PILE_SITE_DTYPE, ascending header then position); pile_info() has the call's figures.  cap: room offered at first (default: one site
        per line); a capacity answer is retried once with the wanted room"""
        lines = pile_lines(lines)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        cap = max(len(lines), 16) if cap is None else int(cap)
        n, info = C.c_uint64(0), np.zeros(8, np.uint64)
        for _ in range(2):
            sites = np.zeros(max(cap, 1), PILE_SITE_DTYPE)
            rc = lib().bhip_pile_run(self._h, _ptr(q.codes), _ptr(q.off), q.n, _ptr(lines), len(lines), _ptr(ops), len(ops), int(min_depth), int(min_alt),
                                     _ptr(sites), cap, C.byref(n), _ptr(info))
            if rc != BHIP_E_CAPACITY or n.value <= cap:
                break
            cap = n.value
        self._pile_info = dict(zip(PILE_INFO, (int(x) for x in info)))
        _chk(rc)
        return sites[:n.value]

    def consensus_run(self, q, lines, ops, min_depth=4, seg_cap=None, letter_cap=None):
        """the consensus of one sample on every position its lines cover (bhip_consensus_run).  q, lines, ops: as pile_run takes them.  Returns
        (segments CONS_SEG_DTYPE in ascending header, position order, letters bytes): segment s owns letters[off : off + len];
        consensus_info() has the call's figures.  seg_cap / letter_cap: room offered at first; a capacity answer is retried once with
        the wanted room"""
        lines = pile_lines(lines)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        seg_cap = max(len(lines), 16) if seg_cap is None else int(seg_cap)
        letter_cap = 1 << 16 if letter_cap is None else int(letter_cap)
        ns, nl, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)
        for _ in range(2):
            segs, letters = np.zeros(max(seg_cap, 1), CONS_SEG_DTYPE), np.zeros(max(letter_cap, 1), np.uint8)
            rc = lib().bhip_consensus_run(self._h, _ptr(q.codes), _ptr(q.off), q.n, _ptr(lines), len(lines), _ptr(ops), len(ops), int(min_depth),
                                          _ptr(segs), seg_cap, C.byref(ns), _ptr(letters), letter_cap, C.byref(nl), _ptr(info))
            if rc != BHIP_E_CAPACITY or (ns.value <= seg_cap and nl.value <= letter_cap):
                break
            seg_cap, letter_cap = max(seg_cap, ns.value), max(letter_cap, nl.value)
        _chk(rc)
        return segs[:ns.value], letters[:nl.value].tobytes()

    def consensus_pairs(self, n_samples, segs, letters, min_compared=1, pair_cap=None, retry=True):
        """every two samples' consensus rows compared per header (bhip_consensus_pairs).  segs: PAIR_SEG_DTYPE, strictly ascending (sample,
        header, pos); letters: the bytes the segments' offsets point into.  Returns the pairs (PAIR_DTYPE, ascending header, a, b) with
        compared >= min_compared; consensus_pairs_info() has the call's figures.  pair_cap: room offered at first; a capacity answer is
        retried once with the number the call asked for -- not with retry=False: the capacity answer is raised, pairs_wanted holds the
        number and pairs_buffer the untouched room"""
        segs, letters = pair_arrays(segs, letters)
        pair_cap = 1024 if pair_cap is None else int(pair_cap)
        for attempt in range(2):
            pairs, n, info = np.zeros(max(pair_cap, 1), PAIR_DTYPE), C.c_uint64(0), np.zeros(8, np.uint64)
            rc = lib().bhip_consensus_pairs(self._h, int(n_samples), _ptr(segs), len(segs), _ptr(letters), len(letters), int(min_compared), _ptr(pairs), pair_cap, C.byref(n), _ptr(info))
            self.pairs_wanted, self.pairs_buffer = int(n.value), pairs
            if rc != BHIP_E_CAPACITY or attempt or not retry:
                break
            pair_cap = int(n.value)
        _chk(rc)
        return pairs[:n.value]

    def consensus_pairs_info(self):
        """the last consensus_pairs' figures (bhip_consensus_pairs_info): segments, headers (with two samples or more), union_positions,
        examined, pairs, device_us, peak_bytes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_consensus_pairs_info(self._h, _ptr(info)))
        return dict(zip(CONS_PAIRS_INFO, (int(x) for x in info)))

    def consensus_info(self):
        """the last consensus_run's figures (bhip_consensus_info): events, candidates, segments, covered, device_us, peak_bytes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_consensus_info(self._h, _ptr(info)))
        return dict(zip(CONS_INFO, (int(x) for x in info)))

    def alleles_run(self, q, lines, ops, min_depth=4, min_alt=2, cap=None, code_cap=None):
        """the indel alleles of one sample (bhip_alleles_run).  q, lines, ops: as pile_run takes them.  Returns (alleles ALLELE_DTYPE in the
        defined order, codes uint8: a Del(n) owns codes[code_off : code_off + n], the reference codes it deletes); alleles_info() has the
        call's figures.  cap / code_cap: room offered at first; a capacity answer is retried once with the wanted room"""
        lines = pile_lines(lines)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        cap = max(len(lines), 16) if cap is None else int(cap)
        code_cap = 1 << 12 if code_cap is None else int(code_cap)
        na, nc, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)
        for _ in range(2):
            out, codes = np.zeros(max(cap, 1), ALLELE_DTYPE), np.zeros(max(code_cap, 1), np.uint8)
            rc = lib().bhip_alleles_run(self._h, _ptr(q.codes), _ptr(q.off), q.n, _ptr(lines), len(lines), _ptr(ops), len(ops), int(min_depth), int(min_alt),
                                        _ptr(out), cap, C.byref(na), _ptr(codes), code_cap, C.byref(nc), _ptr(info))
            if rc != BHIP_E_CAPACITY or (na.value <= cap and nc.value <= code_cap):
                break
            cap, code_cap = max(cap, na.value), max(code_cap, nc.value)
        _chk(rc)
        return out[:na.value], codes[:nc.value]

    def alleles_info(self):
        """the last alleles_run's figures (bhip_alleles_info): events, distinct, alleles, skipped_end, skipped_adjacent, skipped_long, device_us,
        peak_bytes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_alleles_info(self._h, _ptr(info)))
        return dict(zip(ALLELES_INFO, (int(x) for x in info)))

    def site_counts(self, ranges, sites, alleles, records):
        """one sample's counts at the records the caller names (bhip_site_counts).  ranges: COUNT_RANGE_DTYPE, the sample's lines; sites: its
        pile_run(1, 1) result (PILE_SITE_DTYPE, ascending header, pos); alleles: its alleles_run(1, 1) result (ALLELE_DTYPE, in its order);
        records: COUNT_RECORD_DTYPE, in any order.  Returns the cells (COUNT_CELL_DTYPE, one per record); site_counts_info() has the call's
        figures"""
        ranges, sites, alleles, records = count_arrays(ranges, sites, alleles, records)
        cells, info = np.zeros(max(len(records), 1), COUNT_CELL_DTYPE), np.zeros(8, np.uint64)
        _chk(lib().bhip_site_counts(self._h, _ptr(ranges), len(ranges), _ptr(sites), len(sites), _ptr(alleles), len(alleles), _ptr(records), len(records), _ptr(cells), _ptr(info)))
        return cells[:len(records)]

    def site_counts_info(self):
        """the last site_counts' figures (bhip_site_counts_info): ranges, records, device_us, peak_bytes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_site_counts_info(self._h, _ptr(info)))
        return dict(zip(SITE_COUNTS_INFO, (int(x) for x in info)))

    def cluster_run(self, weights, edges):
        """greedy centroid clusters (bhip_cluster_run).  weights: uint32 per node (read), edges: CLUSTER_EDGE_DTYPE array (or rows q, r, edits), raw
        -- duplicates, self edges and edges towards lower priority included.  Returns (centroid uint32 [n], edits uint32 [n]): every node's
        centroid (itself for a centroid) and the edits of the edge that joined it; cluster_info() has the call's figures"""
        weights = np.ascontiguousarray(weights, dtype=np.uint32)
        edges = cluster_edges(edges)
        n = len(weights)
        centroid, edits = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        _chk(lib().bhip_cluster_run(self._h, n, _ptr(weights), _ptr(edges), len(edges), _ptr(centroid), _ptr(edits)))
        return centroid[:n], edits[:n]

    def cluster_info(self):
        """the last cluster_run's figures: rounds, edges_kept, centroids, device_us, device_bytes, edges, nodes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_cluster_info(self._h, _ptr(info)))
        return dict(zip(CLUSTER_INFO, (int(x) for x in info)))

    def chimera_run(self, weights, lens, lines, ops, skew=2, min_seg=16, min_gain=3):
        """the two-parent chimera check (bhip_chimera_run).  weights, lens: uint32 per node (read); lines: CHIM_LINE_DTYPE array (or rows q, r,
        flags, n_ops, op_off), raw -- self lines, lines towards non-candidates and repeated (q, r) included; ops: uint32 words length << 4 |
        code.  Returns a CHIMERA_DTYPE array, one row per node; chimera_info() has the call's figures"""
        weights = np.ascontiguousarray(weights, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        lines = chim_lines(lines)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        n = len(weights)
        if len(lens) != n:
            raise ValueError("chimera_run: one length per weight")
        out = np.zeros(max(n, 1), CHIMERA_DTYPE)
        _chk(lib().bhip_chimera_run(self._h, n, _ptr(weights), _ptr(lens), _ptr(lines), len(lines), _ptr(ops), len(ops), int(skew), int(min_seg), int(min_gain), _ptr(out)))
        return out[:n]

    def chimera_info(self):
        """the last chimera_run's figures: pairs_kept, evaluated, chimeric, device_us, device_bytes, lines, nodes"""
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_chimera_info(self._h, _ptr(info)))
        return dict(zip(CHIMERA_INFO, (int(x) for x in info)))

    def md_tags(self, requests, ref_first, op_off, ops, cap=None):
        """MD strings and NM counts of alignment paths (bhip_md_tags).  requests, ref_first, op_off, ops: what trace_paths took and returned
        (PATH_REQ_DTYPE array or rows q, refIx, finalPos, ed; request i owns ops[op_off[i]:op_off[i + 1]]).  Returns (md uint8 bytes,
        md_off uint64 [n + 1], nm uint32 [n]): request i owns md[md_off[i]:md_off[i + 1]]; md_info() has the call's figures.  cap: room
        offered at first (default: 4 bytes per request and op); a capacity answer is retried once with the wanted room"""
        if not (isinstance(requests, np.ndarray) and requests.dtype == PATH_REQ_DTYPE):
            rows = np.asarray(requests, dtype=np.uint32).reshape(-1, 4)
            requests = np.zeros(len(rows), PATH_REQ_DTYPE)
            for k, name in enumerate(("q", "refIx", "finalPos", "ed")):
                requests[name] = rows[:, k]
        requests = np.ascontiguousarray(requests)
        n = len(requests)
        ref_first, op_off, ops = _arr(ref_first, np.uint32), _arr(op_off, np.uint64), _arr(ops, np.uint32)
        if len(ref_first) < n or len(op_off) != n + 1:
            raise ValueError("md_tags: one ref_first per request, n + 1 offsets")
        cap = 4 * (n + len(ops)) + 16 if cap is None else int(cap)
        md_off, nm, info = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(8, np.uint64)
        for _ in range(2):
            md = np.zeros(max(cap, 1), np.uint8)
            rc = lib().bhip_md_tags(self._h, _ptr(requests), _ptr(ref_first), _ptr(op_off), _ptr(ops), n, _ptr(md), cap, _ptr(md_off), _ptr(nm), _ptr(info))
            if rc != BHIP_E_CAPACITY or int(md_off[n]) <= cap:
                break
            cap = int(md_off[n])
        self._md_info = dict(zip(MD_INFO, (int(x) for x in info)))
        _chk(rc)
        return md[:int(md_off[n])], md_off, nm[:n]

    def md_info(self):
        """the last md_tags call's figures: device_us, requests, md_bytes, peak_bytes"""
        return dict(getattr(self, "_md_info", dict.fromkeys(MD_INFO, 0)))

    def pile_info(self):
        """the last pile_run's figures: events, candidates, sites, device_us, peak_bytes"""
        return dict(getattr(self, "_pile_info", dict.fromkeys(PILE_INFO, 0)))

    def cov_begin(self, lengths, pad=0):
        """coverage over len(lengths) reference headers (bhip_cov_begin); cov_add() one whole sample at a time"""
        lengths = _arr(lengths, np.uint32)
        self._cov_n = len(lengths)
        _chk(lib().bhip_cov_begin(self._h, len(lengths), _ptr(lengths), int(pad)))

    def cov_add(self, sample, lines):
        """lines: COV_LINE_DTYPE array (ref, st, ed, w = weight | unique << 31)"""
        lines = np.ascontiguousarray(lines, dtype=COV_LINE_DTYPE)
        _chk(lib().bhip_cov_add(self._h, int(sample), _ptr(lines), len(lines)))

    def cov_stats(self, sample=None):
        """(shared, unique), each uint64 [headers][4] = tot, cov, sq, lines; sample=None: the Dataset column"""
        sh, un = np.zeros((self._cov_n, 4), np.uint64), np.zeros((self._cov_n, 4), np.uint64)
        if sample is None:
            _chk(lib().bhip_cov_dataset_stats(self._h, _ptr(sh), _ptr(un)))
        else:
            _chk(lib().bhip_cov_sample_stats(self._h, int(sample), _ptr(sh), _ptr(un)))
        return sh, un

    def cov_info(self):
        info = np.zeros(8, np.uint64)
        _chk(lib().bhip_cov_info(self._h, _ptr(info)))
        return dict(zip(("events", "peak_bytes", "compactions", "cap_bytes", "us_last", "events_per_block", "us_total", "samples"), (int(x) for x in info)))

    def cov_end(self):
        _chk(lib().bhip_cov_end(self._h))

    def align_pairs(self, q, pair_q, pair_clump):
        pair_q = _arr(pair_q, np.uint32)
        pair_clump = _arr(pair_clump, np.uint32)
        mins = np.zeros(len(pair_q) * 16, dtype=np.uint8)
        _chk(lib().bhip_align_pairs(self._h, _ptr(q.codes), _ptr(q.off), _ptr(q.emac), q.n, _ptr(pair_q), _ptr(pair_clump),
                                    len(pair_q), _ptr(mins)))
        return mins.reshape(-1, 16)

    def prefilter(self, q, cap=None):
        cap = cap or max(1 << 16, 64 * q.n)
        while True:
            oq = np.zeros(cap, np.uint32)
            oc = np.zeros(cap, np.uint32)
            on = np.zeros(cap, np.uint32)
            n = C.c_uint64()
            rc = lib().bhip_prefilter(self._h, _ptr(q.codes), _ptr(q.off), _ptr(q.emac), q.n, _ptr(oq), _ptr(oc), _ptr(on), cap, C.byref(n))
            if rc == BHIP_E_CAPACITY:
                cap = int(n.value) + 16
                continue
            _chk(rc)
            k = n.value
            return oq[:k], oc[:k], on[:k]


def dna_marks(sym, ref_start, ref_len, W, max_chain=0, max_sh=0, device=0):
    """duplicate marks of one -d DNA partition on the device (bhip_dna_marks): sym = uint8 symbol codes, references at
    [ref_start[r], ref_start[r] + ref_len[r]); returns (flags, max_chain, max_sh, info) with info as include/burst_hip.h lists it"""
    sym = np.ascontiguousarray(sym, np.uint8)
    rs = np.ascontiguousarray(ref_start, np.uint64)
    rl = np.ascontiguousarray(ref_len, np.uint32)
    flags = np.zeros(len(sym), np.uint8)
    info = np.zeros(8, np.uint64)
    mc, ms = C.c_uint64(max_chain), C.c_uint64(max_sh)
    _chk(lib().bhip_dna_marks(device, sym.ctypes.data, len(sym), rs.ctypes.data, rl.ctypes.data, len(rs), W, C.byref(mc), C.byref(ms),
                                flags.ctypes.data, info.ctypes.data))
    return flags, mc.value, ms.value, info
