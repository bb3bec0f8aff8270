"""ctypes binding of the C-ABI in include/ansx.h (libansx.so, built in-tree by csrc/Makefile).

There is no fallback: if the shared library is missing this module raises, and if no gfx950
device is usable ansx_init reports ANSX_ERR_NO_DEVICE.
"""
import ctypes as C
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libansx.so")

FOLD, RFOLD, MSB, INT = 0, 1, 2, 3
FLAG_COMPACT_ALPHABET = 1
OK, ERR_ARG, ERR_CAPACITY, ERR_FORMAT, ERR_HIP, ERR_NO_DEVICE, ERR_DOMAIN, ERR_MODEL = range(8)
BOOL_ALL, BOOL_ANY = 0, 1  # the op of ansx_bool_batch_dev
OCCUR_SHOULD, OCCUR_MUST = 0, 1  # the occur values of ansx_topk_query_batch_dev
FILTER_NOT = 1  # the flag of an ansx_filter_clause (ansx_topk_filter_batch_dev)
FILTER_MAX_COLUMNS, FILTER_MAX_CLAUSES = 64, 16
SINGLE_STREAM = 0xFFFFFFFF
NO_CHECKPOINTS = 0xFFFFFFFF
DEFAULT_BLOCK_INTS = 16384
DEFAULT_CKPT_INTERVAL = 1024
MAX_FIDELITY = 7
GEN_UNIFORM, GEN_GEOMETRIC, GEN_ZIPF = 0, 1, 2
NO_ID = 0xFFFFFFFF  # ansx_next_geq_dev: the id of a target above the last id (its position, n, is what decides)

EXPORTS = [
    "ansx_init", "ansx_destroy", "ansx_strerror", "ansx_last_hip_error", "ansx_codec_name",
    "ansx_bound", "ansx_encode", "ansx_decode", "ansx_encode_dev", "ansx_decode_dev",
    "ansx_container_info", "ansx_profile_enable", "ansx_profile_reset", "ansx_profile_get",
    "ansx_workspace_bytes", "ansx_host_log2", "ansx_selftest_log2", "ansx_selftest_div", "ansx_debug_set",
    "ansx_generate_dev", "ansx_generate_host", "ansx_last_encode_stats", "ansx_merge_containers_dev",
    "ansx_zipf_from_uniform", "ansx_gather_containers", "ansx_last_gather_ranks", "ansx_decode_ranges_dev",
    "ansx_decode_device_ranges_dev", "ansx_decode_batch_dev", "ansx_encode_batch_dev",
    "ansx_decode_batch_ranges_dev", "ansx_decode_sums_dev", "ansx_decode_batch_sums_dev", "ansx_encode_gaps_dev",
    "ansx_encode_batch_gaps_dev", "ansx_block_bases_dev", "ansx_encode_gaps_bases_dev", "ansx_decode_ranges_sums_dev",
    "ansx_decode_device_ranges_sums_dev", "ansx_next_geq_dev", "ansx_encode_batch_gaps_bases_dev",
    "ansx_decode_batch_ranges_sums_dev", "ansx_next_geq_batch_dev", "ansx_last_decode_stats",
    "ansx_intersect_ids_dev", "ansx_intersect_dev", "ansx_intersect_batch_dev", "ansx_union_batch_dev", "ansx_union_dev",
    "ansx_bool_batch_dev", "ansx_last_encode_form", "ansx_topk_batch_dev", "ansx_topk_bool_batch_dev",
    "ansx_topk_query_batch_dev", "ansx_topk_scored_batch_dev", "ansx_topk_facets_batch_dev", "ansx_topk_filter_batch_dev",
    "ansx_decode_batch_device_ranges_dev", "ansx_decode_batch_device_ranges_sums_dev",
]


class Opts(C.Structure):
    _fields_ = [("block_ints", C.c_uint32), ("ckpt_interval", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class Scorer(C.Structure):
    """ansx_scorer: the norms (a byte per document id) and the impact table (tf_rows rows of 256 uint32) of
    ansx_topk_scored_batch_dev, both on the device"""
    _fields_ = [("d_norms", C.c_void_p), ("ndocs", C.c_size_t), ("d_table", C.c_void_p), ("tf_rows", C.c_uint32)]


class Facets(C.Structure):
    """ansx_facets: the column (a uint32 per document id) and the room for nqueries * nvalues counts of
    ansx_topk_facets_batch_dev, both on the device"""
    _fields_ = [("d_values", C.c_void_p), ("ndocs", C.c_size_t), ("nvalues", C.c_uint32), ("d_counts", C.c_void_p)]


class FilterClause(C.Structure):
    """ansx_filter_clause: lo <= column[d] <= hi, or with FILTER_NOT in flags its negation"""
    _fields_ = [("column", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("flags", C.c_uint32)]


class Filters(C.Structure):
    """ansx_filters: the columns (a host array of device addresses, each ndocs uint32) and every query's clauses (host) of
    ansx_topk_filter_batch_dev"""
    _fields_ = [("d_columns", C.c_void_p), ("ncolumns", C.c_uint32), ("ndocs", C.c_size_t), ("clauses", C.c_void_p),
                ("fqoff", C.c_void_p)]


class ContainerHeader(C.Structure):
    _fields_ = [("magic", C.c_uint8 * 6), ("max_present_m1", C.c_uint16), ("kind", C.c_uint32), ("fidelity", C.c_uint32),
                ("n", C.c_uint64), ("block_ints", C.c_uint32), ("ckpt_interval", C.c_uint32),
                ("nblocks", C.c_uint32), ("max_log2_frame", C.c_uint32), ("max_nsyms", C.c_uint32),
                ("ckpts_per_block", C.c_uint32), ("payload_bytes", C.c_uint64),
                ("payload_offset", C.c_uint64)]


class EncodeStats(C.Structure):
    _fields_ = [("max_nsyms", C.c_uint32), ("max_log2_frame", C.c_uint32), ("near_threshold_decisions", C.c_uint32),
                ("path", C.c_uint32), ("host_redecided", C.c_uint32)]


# ansx_decode_stats: the form of the most recent decode (include/ansx.h)
PARSERS = ("DONE", "GENERIC", "PAR", "FAST", "WIN")
DECODERS = ("STAGED", "RING", "SMALL_RING", "PAIR", "TABLE", "GTAB")
DECODE_INDEX_VALIDATED, DECODE_ON_REMEMBERED, DECODE_REPEATED = 1, 2, 4


class DecodeStats(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in (
        "parser", "p_variant", "decoder", "p_grid", "p_threads", "p_lds", "d_grid", "d_threads", "d_lds", "stream_cap",
        "maxM", "max_ns", "max_ep", "max_block_bytes", "nblocks", "flags")]


# ansx_encode_form_report: the forms of the most recent encode (include/ansx.h); the enumerations' names by value
FORM_HIST = ("WORDS", "PACKED", "NONE")
FORM_SORT = ("U16", "U32", "U32_UNSTAGED", "NONE")
FORM_FIN = ("WAVES", "16_5", "16_8", "ONE_WAVE_5", "ONE_WAVE_8", "GENERIC_5", "GENERIC_8", "NONE")
FORM_RF = ("NONE", "HBM_HASH", "LDS_OPT", "LDS_FULL", "SORT")
FORM_PRELUDE = ("W4", "W16", "RANK_SPACE", "GENERIC", "GENERIC_HBM", "NONE")
FORM_ENC = ("INT_STATE", "MODE1", "MODE2", "NONE")
FORM_PC = ("NONE", "A", "B", "C")
FORM_ATTEMPT_BITS = (("optimistic", 1), ("fast_model", 2), ("fused", 4), ("rank_space", 8), ("sp_full_lds", 16), ("batch_pass", 32))


class EncodeFormReport(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in (
        "attempt", "ns_cap", "nt", "hist", "cpb", "h_deferred", "h_in_hist", "sort", "fin", "fcap", "cand_chains", "nranges",
        "range_blocks", "big_geo", "rf", "rf_slots", "pa_small", "pa_slots", "pa_uqcap", "prelude", "table16_first", "pre_cap",
        "enc", "enc_grid", "enc_threads", "enc_lds", "criterion", "pairs", "S", "pc_grid", "first", "nblocks")]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("launches", C.c_uint64)]


def build_library(force=False):
    """Compile csrc/ansx.hip for gfx950 into ans_large_alphabet_amd/libansx.so (hipcc)."""
    args = ["make", "-s", "-C", os.path.join(PKG_DIR, "csrc")]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def _preload_shared_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (SONAME libamdhip64.so.7, same as /opt/rocm's); if libansx.so pulled in
    /opt/rocm's copy first, a later `import torch` would load a second runtime and find no GPU.
    So when torch is installed, load ITS runtime first (without importing torch); libansx.so's
    NEEDED libamdhip64.so.7 then binds to that already-loaded object."""
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # a C++-only deployment simply uses /opt/rocm's runtime


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libansx.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ans_large_alphabet_amd/csrc` (needs hipcc); there is no CPU fallback")
    _preload_shared_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.ansx_init.restype = C.c_int
    L.ansx_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.ansx_destroy.restype = None
    L.ansx_destroy.argtypes = [vp]
    L.ansx_strerror.restype = C.c_char_p
    L.ansx_strerror.argtypes = [C.c_int]
    L.ansx_last_hip_error.restype = C.c_int
    L.ansx_last_hip_error.argtypes = [vp]
    L.ansx_codec_name.restype = C.c_int
    L.ansx_codec_name.argtypes = [C.c_int, C.c_int, C.c_char_p, sz]
    L.ansx_bound.restype = sz
    L.ansx_bound.argtypes = [C.c_int, C.c_int, sz, C.POINTER(Opts)]
    L.ansx_encode.restype = C.c_int
    L.ansx_encode.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Opts)]
    L.ansx_decode.restype = C.c_int
    L.ansx_decode.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(Opts)]
    L.ansx_encode_dev.restype = C.c_int
    L.ansx_encode_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Opts), vp]
    L.ansx_decode_dev.restype = C.c_int
    L.ansx_decode_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(Opts), vp]
    L.ansx_decode_ranges_dev.restype = C.c_int
    L.ansx_decode_ranges_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, vp, sz, vp, sz, vp]
    L.ansx_decode_device_ranges_dev.restype = C.c_int
    L.ansx_decode_device_ranges_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, vp, sz, vp, sz, vp,
                                                C.POINTER(C.c_uint64), vp]
    L.ansx_decode_batch_dev.restype = C.c_int
    L.ansx_decode_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, sz, vp, C.POINTER(C.c_uint64),
                                        C.POINTER(sz), vp]
    L.ansx_decode_batch_ranges_dev.restype = C.c_int
    L.ansx_decode_batch_ranges_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp,
                                               C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_encode_batch_dev.restype = C.c_int
    L.ansx_encode_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, sz, vp, vp, C.POINTER(sz), C.POINTER(sz),
                                        C.POINTER(Opts), vp]
    # running sums and gaps: each takes the arguments of its counterpart
    for name, like in (("ansx_decode_sums_dev", L.ansx_decode_dev), ("ansx_decode_batch_sums_dev", L.ansx_decode_batch_dev),
                       ("ansx_encode_gaps_dev", L.ansx_encode_dev), ("ansx_encode_batch_gaps_dev", L.ansx_encode_batch_dev)):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = list(like.argtypes)
    # docids of ranges: block bases beside the container
    L.ansx_block_bases_dev.restype = C.c_int
    L.ansx_block_bases_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.ansx_encode_gaps_bases_dev.restype = C.c_int
    L.ansx_encode_gaps_bases_dev.argtypes = list(L.ansx_encode_dev.argtypes[:-1]) + [vp, sz, C.POINTER(sz), vp]
    L.ansx_decode_ranges_sums_dev.restype = C.c_int
    L.ansx_decode_ranges_sums_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, vp, vp, sz, vp, sz, vp]
    L.ansx_decode_device_ranges_sums_dev.restype = C.c_int
    L.ansx_decode_device_ranges_sums_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, vp, vp, sz, vp, sz, vp,
                                                     C.POINTER(C.c_uint64), vp]
    # search by value over the bases: targets -> positions and ids
    L.ansx_next_geq_dev.restype = C.c_int
    L.ansx_next_geq_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(C.c_uint64), vp]
    # batches of gap-coded lists: bases from the writer, ids of ranges, search by value
    L.ansx_encode_batch_gaps_bases_dev.restype = C.c_int
    L.ansx_encode_batch_gaps_bases_dev.argtypes = list(L.ansx_encode_batch_dev.argtypes[:-1]) + [vp, sz, vp, C.POINTER(sz), vp]
    L.ansx_decode_batch_ranges_sums_dev.restype = C.c_int
    L.ansx_decode_batch_ranges_sums_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp,
                                                    C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), vp]
    # ... with src / first / cnt in device memory: d_offsets is a device pointer too
    L.ansx_decode_batch_device_ranges_dev.restype = C.c_int
    L.ansx_decode_batch_device_ranges_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp,
                                                      C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_decode_batch_device_ranges_sums_dev.restype = C.c_int
    L.ansx_decode_batch_device_ranges_sums_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, sz,
                                                           vp, C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_next_geq_batch_dev.restype = C.c_int
    L.ansx_next_geq_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp,
                                          C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), vp]
    # intersection: the members of a candidate array in one list; the ids common to several lists
    L.ansx_intersect_ids_dev.restype = C.c_int
    L.ansx_intersect_ids_dev.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, C.POINTER(C.c_uint64), vp]
    L.ansx_intersect_dev.restype = C.c_int
    L.ansx_intersect_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, sz, C.POINTER(C.c_uint64), C.POINTER(sz), vp]
    # ... of many queries over one batch in one call
    L.ansx_intersect_batch_dev.restype = C.c_int
    L.ansx_intersect_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, vp, sz, vp, sz, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_union_batch_dev.restype = C.c_int
    L.ansx_union_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_bool_batch_dev.restype = C.c_int
    L.ansx_bool_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, C.c_int, vp, vp, vp, vp, sz, vp, sz, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_batch_dev.restype = C.c_int
    L.ansx_topk_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, sz, C.c_uint32, vp, vp, vp,
                                      C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_bool_batch_dev.restype = C.c_int
    L.ansx_topk_bool_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, C.c_int, vp, vp, vp, vp, vp, sz, C.c_uint32,
                                           vp, vp, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_query_batch_dev.restype = C.c_int
    L.ansx_topk_query_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, C.c_uint32,
                                            vp, vp, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_scored_batch_dev.restype = C.c_int
    L.ansx_topk_scored_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Scorer), sz,
                                             C.c_uint32, vp, vp, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_facets_batch_dev.restype = C.c_int
    L.ansx_topk_facets_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Scorer),
                                             C.POINTER(Facets), sz, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz), vp]
    L.ansx_topk_filter_batch_dev.restype = C.c_int
    L.ansx_topk_filter_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Scorer),
                                             C.POINTER(Facets), C.POINTER(Filters), sz, C.c_uint32, vp, vp, vp, vp, C.POINTER(sz),
                                             C.POINTER(sz), vp]
    L.ansx_union_dev.restype = C.c_int
    L.ansx_union_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(sz), vp]
    L.ansx_container_info.restype = C.c_int
    L.ansx_container_info.argtypes = [vp, sz, C.POINTER(ContainerHeader)]
    L.ansx_profile_enable.restype = C.c_int
    L.ansx_profile_enable.argtypes = [vp, C.c_int]
    L.ansx_profile_reset.restype = C.c_int
    L.ansx_profile_reset.argtypes = [vp]
    L.ansx_profile_get.restype = C.c_int
    L.ansx_profile_get.argtypes = [vp, C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]
    L.ansx_workspace_bytes.restype = sz
    L.ansx_workspace_bytes.argtypes = [vp]
    L.ansx_generate_dev.restype = C.c_int
    L.ansx_generate_dev.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, vp, sz, vp]
    L.ansx_generate_host.restype = C.c_int
    L.ansx_generate_host.argtypes = [C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, vp, sz]
    L.ansx_merge_containers_dev.restype = C.c_int
    L.ansx_merge_containers_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.c_int, vp, sz, C.POINTER(sz), vp]
    L.ansx_last_encode_stats.restype = C.c_int
    L.ansx_last_encode_stats.argtypes = [vp, C.POINTER(EncodeStats)]
    L.ansx_last_encode_form.restype = C.c_int
    L.ansx_last_encode_form.argtypes = [vp, C.POINTER(EncodeFormReport)]
    L.ansx_last_decode_stats.restype = C.c_int
    L.ansx_last_decode_stats.argtypes = [vp, C.POINTER(DecodeStats)]
    L.ansx_last_gather_ranks.restype = C.c_int
    L.ansx_last_gather_ranks.argtypes = [vp]
    L.ansx_debug_set.restype = C.c_int
    L.ansx_debug_set.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.ansx_zipf_from_uniform.restype = C.c_int
    L.ansx_zipf_from_uniform.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.ansx_host_log2.restype = C.c_double
    L.ansx_host_log2.argtypes = [C.c_double]
    L.ansx_selftest_log2.restype = C.c_int
    L.ansx_selftest_log2.argtypes = [vp, vp, vp, sz]
    L.ansx_selftest_div.restype = C.c_int
    L.ansx_selftest_div.argtypes = [vp, vp, vp, vp, sz]
    _lib = L
    return L


class AnsxError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().ansx_strerror(status).decode()
        super().__init__("%s: %s (status %d)" % (what, msg, status))
